// kfamd_kernels.h — C ABI of the hand-written CDNA4 (gfx950) kernel library.
//
// This library is the MI355X compute path of the framework (SURVEY.md §2.7.2, K1–K3):
//   K1  bf16 GEMM on MFMA (v_mfma_f32_16x16x32_bf16), LDS-tiled, global_load_lds staging
//   K2  LayerNorm / RMSNorm forward+backward (bf16 I/O, fp32 statistics)
//   K3  one-shot peer all-reduce for small messages (allreduce_oneshot.hip); large messages
//       go to RCCL (native/readiness, kubeflow_rm_amd.parallel)
//
// It is consumed three ways, all in-tree:
//   * Python (kubeflow_rm_amd.ops) through ctypes — one HIP runtime shared with torch;
//   * the native in-pod readiness op (native/readiness) linked directly;
//   * the bench harness (bench.py) through the Python ops.
//
// Every launcher is asynchronous on the given stream and never allocates, syncs or copies,
// so callers may capture it into a hipGraph (cdna_hip_programming.md §6 G9).
// Return value: 0 on success, otherwise a negative kfamd_status code (shape/alignment
// contract violated) or a positive hipError_t from the launch.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum kfamd_status {
  KFAMD_OK = 0,
  KFAMD_EINVAL = -1,     // bad shape / null pointer
  KFAMD_EALIGN = -2,     // pointer or leading dimension not 16-byte aligned for the fast path
};

// Epilogue activation codes for the fused GEMM epilogue.
enum kfamd_act { KFAMD_ACT_NONE = 0, KFAMD_ACT_RELU = 1, KFAMD_ACT_GELU_TANH = 2, KFAMD_ACT_SILU = 3 };

// C[b][m][n] = act(alpha * sum_k A[b][m][k] * B[b][n][k] + bias[n]) (+ R[b][m][n])
//   A: [batch][M][K] row-major (lda, stride_a in elements), K contiguous
//   B: [batch][N][K] row-major (ldb, stride_b), K contiguous   -> "NT" (== torch F.linear)
//   C: [batch][M][N] row-major (ldc, stride_c)
//   bias: optional [N] bf16 (nullptr = none); R: optional residual, same layout as C (ldr/stride_r)
// Dispatch: the 256x256x64 MFMA tile kernel when M%256==0, N%256==0, K%64==0 and all
// pointers/leading dims are 16-byte aligned; otherwise the bounds-checked 128x128 kernel.
int kfamd_gemm_nt_bf16(const void* A, const void* B, void* C, const void* bias, const void* R,
                       int M, int N, int K, int batch,
                       long long lda, long long ldb, long long ldc, long long ldr,
                       long long stride_a, long long stride_b, long long stride_c, long long stride_r,
                       float alpha, int act, void* stream);

// Force a specific kernel (for tests/bench): variant 0 = auto, 1 = 256x256 fast path, 2 = generic.
int kfamd_gemm_nt_bf16_variant(int variant, const void* A, const void* B, void* C, const void* bias,
                               const void* R, int M, int N, int K, int batch,
                               long long lda, long long ldb, long long ldc, long long ldr,
                               long long stride_a, long long stride_b, long long stride_c,
                               long long stride_r, float alpha, int act, void* stream);

// Layout-general GEMM on the w4 MFMA template: C[b][m][n] = act(alpha * sum_k Aop[m][k] Bop[n][k]
// + bias[n]) (+ R), with
//   la = 0: A stored [M][K] (K contiguous, lda >= K)   la = 1: A stored [K][M] (M contiguous, lda >= M)
//   lb = 0: B stored [N][K] (K contiguous, ldb >= K)   lb = 1: B stored [K][N] (N contiguous, ldb >= N)
// Aux (la = lb = 0, act = gelu/silu only): second output with the pre-activation (same layout as C).
// Transposed layouts take only alpha and R (R may alias C: C += A.B). Edge tiles are handled in the
// kernel (any M, N >= 128; N % 8; K % 8 when an operand is K-contiguous; M % 8 when la = 1). Other
// shapes return KFAMD_EINVAL and the caller falls back.
int kfamd_gemm_bf16_ex(int la, int lb, const void* A, const void* B, void* C, const void* bias, const void* R,
                       void* Aux, int M, int N, int K, int batch, long long lda, long long ldb, long long ldc,
                       long long ldr, long long stride_a, long long stride_b, long long stride_c, long long stride_r,
                       float alpha, int act, void* stream);

// Split-K for problems with too few 128x128 output tiles to fill the chip: the partial products
// of K range [z*kper, (z+1)*kper) go to W[z][b][M][N] fp32 (kper % 64 == 0, splits*kper >= K),
// then kfamd_splitk_reduce applies the epilogue into bf16 C. Same shape contract as _ex at bm=128.
int kfamd_w4_splitk_nt(const void* A, const void* B, float* W, int M, int N, int K, int batch, int splits, int kper,
                       long long lda, long long ldb, long long stride_a, long long stride_b, void* stream);
int kfamd_w4_splitk_t(int la, int lb, const void* A, const void* B, float* W, int M, int N, int K, int batch,
                      int splits, int kper, long long lda, long long ldb, long long stride_a, long long stride_b,
                      void* stream);
// Stream-K (256 tile, NT, batch 1) for grids whose last wave would leave CUs idle: `grid` persistent
// blocks (one per CU), the rem = tiles % grid leftover tiles in `splits` K-splits each; W = (splits -
// 1) * rem x 256 x 256 fp32, flags = splits * rem words owned by the calling stream with a strictly
// increasing non-zero epoch per call. Epilogues as kfamd_w4_launch_nt without the Aux output.
int kfamd_w4_streamk_nt(const void* A, const void* B, void* C, const void* bias, const void* R, void* Aux, int M,
                        int N, int K, long long lda, long long ldb, long long ldc, long long ldr, float alpha, int act,
                        float* W, unsigned* flags, unsigned epoch, int grid, int splits, void* stream);
int kfamd_splitk_reduce(const float* W, void* C, const void* bias, const void* R, void* Aux, int M, int N, int batch,
                        int splits, long long ldc, long long ldr, long long stride_c, long long stride_r, float alpha,
                        int act, void* stream);

// Softmax cross-entropy (xent_bf16.hip): forward -> per-row loss and log-sum-exp (fp32); backward ->
// dlogits = (softmax - onehot) * (*g / *count) in bf16 (device scalars: no host sync).
int kfamd_xent_fwd_bf16(const void* logits, long long ld, const long long* target, float* loss, float* lse, int rows,
                        int V, long long ignore_index, void* stream);
int kfamd_xent_bwd_bf16(const void* logits, long long ld, const long long* target, const float* lse, void* grad,
                        long long ldg, int rows, int V, long long ignore_index, const float* g, const float* count,
                        void* stream);

// K-padding pack (pad_bf16.hip): dst_i[r][0:Kp] = src_i[r][0:K], zero tail, both GEMM operands in
// one launch (rows1 = 0: one matrix). Kp % 8 == 0; dst dense and 16-B aligned.
int kfamd_pad_k_bf16(const void* src0, void* dst0, long long rows0, long long ld0, const void* src1, void* dst1,
                     long long rows1, long long ld1, int K, int Kp, void* stream);

// Fused linear-backward tail: g = dy * act'(z) (bf16; z = the forward's Aux pre-activation, or its
// output y for relu), db = column sums of g (fp32, optional). act == NONE: only db = sum over rows of
// dy (g unused). [rows][cols], cols % 8 == 0, 16-B aligned. workspace: kfamd_act_grad_workspace bytes.
long long kfamd_act_grad_workspace(int rows, int cols);
// y = act(z) elementwise (n % 8 == 0, 16-B aligned): the forward activation as its own pass
int kfamd_act_fwd_bf16(const void* z, void* y, long long n, int act, void* stream);
// multi-tensor AdamW over bf16 params / grads / moments, one launch per step (kernels/adamw_bf16.hip)
int kfamd_adamw_tensor_bytes(void);
int kfamd_adamw_chunk(void);
int kfamd_adamw_bf16(const void* table, const void* owner, long long nchunks, float lr, float b1, float b2, float eps,
                     float wd, float step_size, float inv_sqrt_bc2, void* stream);
// attention backward: dq / dk / dv [B][H][T][D] (strided) packed into the fused QKV gradient
// [B][T][3][H][D] in one pass (kernels/qkv_pack_bf16.hip)
int kfamd_qkv_pack_bf16(const void* dq, const void* dk, const void* dv, void* out, int B, int T, int H, int D,
                        long long qb, long long qh, long long qt, long long kb, long long kh, long long kt,
                        long long vb, long long vh, long long vt, void* stream);
int kfamd_act_grad_bf16(const void* dy, const void* z, void* g, float* db, float* workspace, int rows, int cols,
                        int act, void* stream);
// the same with db written as bf16 when db_bf16 (fp32 accumulation)
int kfamd_act_grad_bf16_v2(const void* dy, const void* z, void* g, void* db, int db_bf16, float* workspace, int rows,
                           int cols, int act, void* stream);
// db[c] = sum over b < nblk of ws[b][c] (fp32 partials; db fp32, or bf16 when db_bf16)
int kfamd_colsum_finalize(const float* ws, void* db, int db_bf16, int nblk, int cols, void* stream);
// A linear layer's dgrad through the previous layer's activation, one GEMM (gemm_w4.h DACT):
// G[M][N] = (dY[M][K] . W[K][N]) * act'(Z[M][N]) (dY K-contiguous with row stride lda, W row-major
// [K][N] with row stride ldb, Z / G row strides ldz / ldg), and when db is given the column sums of G
// (the previous layer's bias gradient; ws: kfamd_w4_dgrad_act_workspace bytes). M, N multiples of
// 256, K of 64, 16-B rows; KFAMD_EINVAL otherwise (callers fall back to the GEMM + act-grad pass).
// Two weight gradients in one launch: C_i[M_i][N] = A_i^T . B_i, A_i [K][M_i] (row stride lda_i), B_i
// [K][N] (ldb_i), C_i row stride ldc_i (kernels/tu/w4_wgrad_pair.hip).
int kfamd_w4_wgrad_pair(const void* A1, const void* B1, void* C1, int M1, long long lda1, long long ldb1,
                        long long ldc1, const void* A2, const void* B2, void* C2, int M2, long long lda2,
                        long long ldb2, long long ldc2, int N, int K, void* stream);
// the same with problem 2's own width N2 and, for splits > 1, K split in kper pieces with the in-kernel
// fixup (W: splits x tiles fp32 256 x 256 partials, cnt: tiles arrival counters, zero on entry and exit)
int kfamd_w4_wgrad_pair_v2(const void* A1, const void* B1, void* C1, int M1, long long lda1, long long ldb1,
                           long long ldc1, const void* A2, const void* B2, void* C2, int M2, long long lda2,
                           long long ldb2, long long ldc2, int N, int N2, int K, int splits, int kper, float* W,
                           unsigned* cnt, void* stream);
long long kfamd_w4_dgrad_act_workspace(int M, int N);
int kfamd_w4_dgrad_act(const void* dy, const void* w, void* g, const void* z, int M, int N, int K, long long lda,
                       long long ldb, long long ldg, long long ldz, int act, float* ws, void* db, int db_bf16,
                       void* stream);

// LayerNorm forward over the last dim (hidden). x,y: [rows][hidden] bf16 (row stride = hidden).
// gamma/beta: [hidden] bf16 (beta may be null). mean/rstd: optional fp32 [rows] (saved for bwd).
int kfamd_layernorm_fwd_bf16(const void* x, const void* gamma, const void* beta, void* y,
                             float* mean, float* rstd, int rows, int hidden, float eps, void* stream);

// RMSNorm forward: y = x * rsqrt(mean(x^2)+eps) * gamma. rstd optional.
int kfamd_rmsnorm_fwd_bf16(const void* x, const void* gamma, void* y, float* rstd,
                           int rows, int hidden, float eps, void* stream);

// The two forwards with the launch path forced (tests / bench); rms != 0: RMSNorm (beta and mean are ignored).
//   path 0: the launcher's rule   1: one-shot wave per row (hidden 512 * {1,2,3,4,5,6,8,10,12,16} on 16-B pointers,
//   256 * {1,3,5} on 8-B pointers)   2: streaming (hidden 512 * {1,2,3,4,5,6,8} double-buffered, 8192 rolling reload;
//   16-B pointers)   3: one workgroup per row (any hidden, any alignment)
//   blocks: the streaming kernel's grid in workgroups of 4 waves, 0 = the launcher's.
// A path the shape or the alignment cannot take, a path outside 0 .. 3 or blocks < 0: KFAMD_EINVAL, nothing launched.
int kfamd_norm_fwd_bf16_path(int rms, int path, int blocks, const void* x, const void* gamma, const void* beta, void* y,
                             float* mean, float* rstd, int rows, int hidden, float eps, void* stream);
// the path (1 .. 3) that path 0 takes for this shape on 16-B aligned pointers on the current device; KFAMD_EINVAL
// for rows or hidden < 1
int kfamd_norm_fwd_path_for(int rms, int rows, int hidden);

// LayerNorm backward. dx: [rows][hidden] bf16. dgamma/dbeta: fp32 [hidden] (fully written).
// workspace: fp32 scratch of kfamd_layernorm_bwd_workspace(rows, hidden) bytes.
long long kfamd_layernorm_bwd_workspace(int rows, int hidden);
int kfamd_layernorm_bwd_bf16(const void* dy, const void* x, const void* gamma, const float* mean,
                             const float* rstd, void* dx, float* dgamma, float* dbeta,
                             float* workspace, int rows, int hidden, void* stream);
// the same with dgamma / dbeta written as bf16 when dgb_bf16 (fp32 accumulation)
// v3: dres (optional, [rows][hidden] bf16, not aliasing dx): dx = dres + the LayerNorm input
// gradient (a pre-norm residual stream's two gradient contributions in one store)
int kfamd_layernorm_bwd_bf16_v3(const void* dy, const void* dres, const void* x, const void* gamma,
                                const float* mean, const float* rstd, void* dx, void* dgamma, void* dbeta,
                                int dgb_bf16, float* workspace, int rows, int hidden, void* stream);
int kfamd_layernorm_bwd_bf16_v2(const void* dy, const void* x, const void* gamma, const float* mean,
                                const float* rstd, void* dx, void* dgamma, void* dbeta, int dgb_bf16,
                                float* workspace, int rows, int hidden, void* stream);

// ---- K3: one-shot all-reduce over peer-visible buffers ------------------------------------------
enum kfamd_dtype { KFAMD_DTYPE_F32 = 0, KFAMD_DTYPE_BF16 = 1 };
// out[r] = sum over ranks of in[*] (fp32 accumulation in rank order: bit-identical on every rank).
// inputs/flags: nranks pointers (peer-visible: same device, peer-access or IPC-opened), 16-B
// aligned; outputs: rank-indexed, only [rank0, rank0 + launch_ranks) are written. One launch serves
// launch_ranks ranks (1 per device in real use; several to simulate ranks on one GPU). flags[r]:
// kfamd_allreduce_oneshot_flag_bytes(nranks, nblocks) zeroed bytes per rank, reused across calls
// with epoch = 1, 2, 3, ... (same nblocks every call). *timeout is set if a peer never arrived.
long long kfamd_allreduce_oneshot_flag_bytes(int nranks, int nblocks);
int kfamd_allreduce_oneshot_blocks(long long n, int dtype);
// Barrier deadline per call (default 5000 ms); a missed deadline sets *timeout and NaN-poisons the output.
void kfamd_allreduce_oneshot_set_timeout_ms(int ms);
int kfamd_allreduce_oneshot(const void* const* inputs, void* const* outputs, uint32_t* const* flags,
                            int nranks, int rank0, int launch_ranks, long long n, int dtype,
                            unsigned epoch, int nblocks, unsigned* timeout, void* stream);

// Two-shot (reduce-scatter + all-gather) for mid-size messages: inputs peer-visible
// and overwritten in place (rank r's slice r becomes the reduced slice), outputs per rank (need not be
// peer-visible). Same flags / epochs / timeout contract as the one-shot (flag arrays are shared).
int kfamd_allreduce_twoshot_blocks(long long n, int dtype, int nranks);
int kfamd_allreduce_twoshot(void* const* inputs, void* const* outputs, uint32_t* const* flags, int nranks, int rank0,
                            int launch_ranks, long long n, int dtype, unsigned epoch, int nblocks, unsigned* timeout,
                            void* stream);

// HIP IPC registration for one-process-per-GPU ranks (64-byte handles exchanged by the caller).
int kfamd_ipc_alloc(long long bytes, int uncached, void** ptr, void* handle64);
int kfamd_ipc_open(const void* handle64, void** ptr);
int kfamd_ipc_close(void* ptr);
int kfamd_ipc_free(void* ptr);
int kfamd_copy_async(void* dst, const void* src, long long bytes, void* stream);

// Library identity (for the loud "native code loaded" check).
const char* kfamd_build_info(void);

// Flash attention (attention_bf16.hip), bf16 I/O, fp32 softmax, head dim D = 64 or 128.
// Tensors are [B][H][T][D] views with element strides (b, h, t) (multiples of 8) and D contiguous;
// strides[3 * i + {0, 1, 2}] for tensor i in the order q, k, v, o (forward) or q, k, v, o, do, dq,
// dk, dv (backward). lse: f32 [B][H][T] (written by the forward, read by the backward).
// causal: key <= query. The backward's `workspace` (kfamd_attn_bwd_workspace bytes) holds
// the row constants -lse / scale and -delta, f32 [B][H][T] each, that its dQ kernel writes for its dK / dV kernel; it
// need not be zeroed.
int kfamd_attn_fwd_bf16(const void* q, const void* k, const void* v, void* o, void* lse, int B, int H, int T,
                        int D, float scale, int causal, const long long* strides, void* stream);
long long kfamd_attn_bwd_workspace(int B, int H, int T, int D);
int kfamd_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout,
                        const void* lse, void* dq, void* dk, void* dv, void* workspace, int B, int H, int T,
                        int D, float scale, int causal, const long long* strides, void* stream);
// Grouped-query attention on the same kernels: k, v (and dk, dv) are [B][Hkv][T][D] views with Hkv dividing H;
// query head h reads K / V head h / G, G = H / Hkv (the Llama convention of the KV-cache kernels), in place: no
// expanded copy. q, o, do, dq and lse keep H heads; the grids of the forward and of dQ stay in query heads, so a
// query head does the arithmetic it does on K / V expanded to H heads, bit for bit. dK / dV: one workgroup sweeps
// the query tiles of GS query heads of a group (GS divides G) and sums them in fp32 registers. GS = G stores
// bf16 directly; GS < G writes fp32 parts to the workspace and a reduce kernel adds them in a fixed order (no
// atomics: both routes are deterministic). group_split: the GS to use, 0 = the launcher's rule, which
// kfamd_attn_bwd_gqa_group_split returns (the largest divisor of G whose grid ceil(T / 128) * Hkv * B * (G / GS)
// has 1.5 workgroups per slot, slots = compute units x (D == 64 ? 2 : 1), else 1). kfamd_attn_bwd_gqa_workspace: bytes for that group_split.
// Hkv == H is kfamd_attn_fwd_bf16 / kfamd_attn_bwd_bf16: the same kernels, grids and bits.
// KFAMD_EINVAL (group_split / workspace: a negative value): Hkv < 1, H % Hkv != 0, a group_split that does not
// divide G, and Hkv != H in a build whose backward is not the default schedule (the A/B macros of the .hip).
int kfamd_attn_fwd_gqa_bf16(const void* q, const void* k, const void* v, void* o, void* lse, int B, int H, int Hkv,
                            int T, int D, float scale, int causal, const long long* strides, void* stream);
int kfamd_attn_bwd_gqa_group_split(int B, int H, int Hkv, int T, int D);
long long kfamd_attn_bwd_gqa_workspace(int B, int H, int Hkv, int T, int D, int group_split);
int kfamd_attn_bwd_gqa_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout,
                            const void* lse, void* dq, void* dk, void* dv, void* workspace, int B, int H, int Hkv,
                            int T, int D, float scale, int causal, int group_split, const long long* strides,
                            void* stream);

// ---- decode (KV-cache generation) ------------------------------------------------------------
// Everything from here to the FP8 entry points is attn_kv.hip.
// Single-query attention over a KV cache, bf16 I/O, fp32 softmax, D = 64 / 128.
//   q [B][H][D] (element strides b, h), k_cache / v_cache [B][H][Tcap][D] (strides b, h, t),
//   o [B][H][D] (strides b, h); head dim contiguous. strides = {qb, qh, kb, kh, kt, vb, vh, vt, ob, oh}.
//   lens: DEVICE int32 [B]; row b attends keys 0 .. lens[b]-1 (clamped to t_bound). t_bound: host upper
//   bound of every lens[b] (<= Tcap); it sizes the grid: ceil(t_bound / split_keys) splits per (b, h).
//   lse: optional f32 [B][H]. ws: kfamd_attn_decode_workspace bytes (unused with one split).
// KFAMD_EINVAL: D not 64 / 128, t_bound < 1, a (b, h) slice of 2^31 bytes or more; KFAMD_EALIGN: rows
// not 16-B aligned.
int kfamd_attn_decode_split_keys(void);
long long kfamd_attn_decode_workspace(int B, int H, int D, int t_bound);
int kfamd_attn_decode_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                           float* lse, void* ws, int B, int H, int D, int t_bound, float scale,
                           const long long* strides, void* stream);
// Multi-query attention over the KV cache: Tq (1 .. 16) new rows per (b, h), already appended to
// the cache; K / V are streamed once per (b, h, split) for up to 8 rows (two split launches
// for Tq = 9 .. 16).
//   q, o [B][Tq][H][D] (element strides b, t, h; head dim contiguous), caches as for decode.
//   strides = {qb, qt, qh, kb, kh, kt, vb, vh, vt, ob, ot, oh}.
//   lens: DEVICE int32 [B], the number of keys INCLUDING the Tq new rows (clamped to [0, t_bound]); query
//   row i attends keys 0 .. lens[b] - Tq + i. A row whose limit is negative (lens[b] < Tq) writes zeros
//   and lse = -inf. lse: optional f32 [B][Tq][H]. ws: kfamd_attn_extend_workspace bytes (Tq times
//   decode's; unused with one split). Return codes as kfamd_attn_decode_bf16, plus KFAMD_EINVAL for Tq
//   outside 1 .. 16 and for a missing workspace with more than one split.
long long kfamd_attn_extend_workspace(int B, int H, int D, int Tq, int t_bound);
int kfamd_attn_extend_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                           float* lse, void* ws, int B, int H, int D, int Tq, int t_bound, float scale,
                           const long long* strides, void* stream);
// K and V rows of a fused QKV activation [B][T][3][H][D] (element strides qb, qt; [3][H][D] dense) into
// the caches at rows pos[b] .. pos[b]+T-1 (pos: device int32 [B], not advanced). cache_strides = {kb, kh,
// kt, vb, vh, vt}. Rows at or beyond Tcap are dropped.
int kfamd_kv_append_bf16(const void* qkv, void* k_cache, void* v_cache, const int* pos, int B, int T, int H, int D,
                         int Tcap, long long qb, long long qt, const long long* cache_strides, void* stream);

// ---- FP8 KV cache (attn_kv.hip) ---------------------------------------------------------------
// The cache stored as OCP e4m3fn codes [B][H][Tcap][D] (one byte per element, strides b, h, t in
// elements = bytes, multiples of 16; base 16-B aligned) with one fp32 scale per stored row: k_scale /
// v_scale [B][H][Tcap] (strides b, h in elements; positions contiguous). A row x[0..D) of bf16 values is
// stored as scale = max|x| / 448 (1 for an all-zero row) and code = RNE_e4m3(clamp(x / scale, +-448));
// code * scale gives it back. D = 64 / 128.
// kfamd_kv_append_fp8: the K and V rows of a fused QKV activation, as kfamd_kv_append_bf16, quantised on
//   the way. cache_strides = {kb, kh, kt, vb, vh, vt, ksb, ksh, vsb, vsh}. Rows at or beyond Tcap are
//   dropped: neither codes nor scale are written. Any T.
// kfamd_attn_decode_fp8 / kfamd_attn_extend_fp8: the FP8-cache forms of kfamd_attn_decode_bf16 /
//   kfamd_attn_extend_bf16: bf16 q and o, the same lens / t_bound / lse / workspace contract (the workspace
//   sizes are kfamd_attn_decode_workspace / kfamd_attn_extend_workspace) and the same return codes. The
//   score of key j is (q . codes_k[j]) * k_scale[j]; v_scale[j] is folded into p. Codes and scales at or
//   beyond lens[b] are never used (they may be NaN).
//   decode strides = {qb, qh, kb, kh, kt, vb, vh, vt, ob, oh, ksb, ksh, vsb, vsh};
//   extend strides = {qb, qt, qh, kb, kh, kt, vb, vh, vt, ob, ot, oh, ksb, ksh, vsb, vsh}.
int kfamd_kv_append_fp8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale, const int* pos,
                        int B, int T, int H, int D, int Tcap, long long qb, long long qt,
                        const long long* cache_strides, void* stream);
int kfamd_attn_decode_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                          const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H, int D,
                          int t_bound, float scale, const long long* strides, void* stream);
int kfamd_attn_extend_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                          const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H, int D,
                          int Tq, int t_bound, float scale, const long long* strides, void* stream);

// ---- chunked-prefill attention (attn_kv_mfma.hip) ---------------------------------------------
// kfamd_attn_extend_bf16 / _fp8 without the row limit, on MFMA query tiles: Tq (1 .. 65535) new rows per
// (b, h), already appended to the cache; the same tensors, stride arrays, lens / t_bound contract (row i
// attends keys 0 .. lens[b] - Tq + i; a negative limit writes zeros and lse = -inf; nothing at or beyond
// lens[b] is used), lse [B][Tq][H] and return codes. One workgroup takes kfamd_attn_chunk_tile_rows() query
// rows of one (b, h) and one split of the keys.
//   kfamd_attn_chunk_nsplit: the launcher's split count, from host values only: with tiles = ceil(Tq /
//     tile_rows), clamp(ceil(256 / (tiles * H * B)), 1, ceil(t_bound / split_keys)); 0 for a rejected shape.
//     It does not fall when t_bound grows.
//   kfamd_attn_chunk_workspace: bytes of ws for that split count, B * H * Tq * nsplit * (D + 2) * 4 (below
//     2 * 256 * tile_rows * (D + 2) * 4: 34.1 MB at D = 128); 16 with one split, where ws is unused and may
//     be null; 0 for a rejected shape (D not 64 / 128, Tq outside 1 .. 65535, t_bound < 1).
int kfamd_attn_chunk_tile_rows(void);
int kfamd_attn_chunk_nsplit(int B, int H, int Tq, int t_bound);
long long kfamd_attn_chunk_workspace(int B, int H, int D, int Tq, int t_bound);
int kfamd_attn_chunk_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                          float* lse, void* ws, int B, int H, int D, int Tq, int t_bound, float scale,
                          const long long* strides, void* stream);
int kfamd_attn_chunk_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                         const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H, int D,
                         int Tq, int t_bound, float scale, const long long* strides, void* stream);

// ---- grouped-query attention over the KV cache (attn_kv.hip, attn_kv_mfma.hip) -----------------
// Hkv K / V heads, G = Hq / Hkv query heads on each: query head h reads K / V head h / G (the Llama
// convention). G in {1, 2, 4, 8, 16}; G = 1 launches exactly what the entry points above launch.
//   q, o [B][T][Hq][D] and lse [B][T][Hq] as above, their h strides running over the Hq = Hkv * G query heads;
//   the caches [B][Hkv][Tcap][D] and the FP8 scales [B][Hkv][Tcap]; the stride arrays of the extend / chunk
//   entry points above. A step of T tokens is T * G rows per (b, K / V head), flattened token-major
//   (r = t * G + g): row r is token r / G of query head hkv * G + r % G and attends keys
//   0 .. lens[b] - T + r / G. lens, t_bound, the negative-limit rule (zeros, lse = -inf) and the rule that
//   nothing at or beyond lens[b] is used are unchanged.
//   kfamd_attn_extend_gqa_*: T * G <= 16 rows (K / V streamed once per 8 rows); single-token decode is T = 1
//     with t strides of 0. Workspace: kfamd_attn_extend_gqa_workspace = decode's for Hkv heads times T * G.
//   kfamd_attn_chunk_gqa_*: T * G <= 65535 rows on the MFMA tiles of 128 rows; the split count is
//     kfamd_attn_chunk_nsplit's rule with tiles = ceil(T * G / 128) and H := Hkv, the workspace
//     B * Hkv * (T * G) * nsplit * (D + 2) * 4 bytes (16 with one split).
//   kfamd_kv_append_gqa_*: the fused QKV activation is [B][T][(Hq + 2 Hkv) D], q: Hq D | k: Hkv D | v: Hkv D
//     (element strides qb, qt); the Hkv K and V heads go to the caches as in kfamd_kv_append_bf16 / _fp8.
// Return codes as above; KFAMD_EINVAL (before any KFAMD_EALIGN) also for G outside {1, 2, 4, 8, 16} (Hq no
// such multiple of Hkv), T * G > 16 in the extend form and T * G > 65535 in the chunk form. The workspace
// and nsplit queries return 0 for a rejected shape.
long long kfamd_attn_extend_gqa_workspace(int B, int Hkv, int G, int D, int T, int t_bound);
int kfamd_attn_extend_gqa_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                               float* lse, void* ws, int B, int Hkv, int G, int D, int T, int t_bound, float scale,
                               const long long* strides, void* stream);
int kfamd_attn_extend_gqa_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                              const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int Hkv,
                              int G, int D, int T, int t_bound, float scale, const long long* strides, void* stream);
int kfamd_attn_chunk_gqa_nsplit(int B, int Hkv, int G, int T, int t_bound);
long long kfamd_attn_chunk_gqa_workspace(int B, int Hkv, int G, int D, int T, int t_bound);
int kfamd_attn_chunk_gqa_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                              float* lse, void* ws, int B, int Hkv, int G, int D, int T, int t_bound, float scale,
                              const long long* strides, void* stream);
int kfamd_attn_chunk_gqa_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                             const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int Hkv,
                             int G, int D, int T, int t_bound, float scale, const long long* strides, void* stream);
int kfamd_kv_append_gqa_bf16(const void* qkv, void* k_cache, void* v_cache, const int* pos, int B, int T, int Hq,
                             int Hkv, int D, int Tcap, long long qb, long long qt, const long long* cache_strides,
                             void* stream);
int kfamd_kv_append_gqa_fp8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                            const int* pos, int B, int T, int Hq, int Hkv, int D, int Tcap, long long qb, long long qt,
                            const long long* cache_strides, void* stream);

// ---- sliding-window attention over the KV cache (attn_kv.hip, attn_kv_mfma.hip) -----------------------
// The entry points above with a local causal mask: a row whose causal limit is L (it sees keys 0 .. L - 1 above:
// L = lens[b] for decode, lens[b] - T + t + 1 for row t of T, the token's for a grouped row) sees key j iff
// max(0, L - window) <= j < L: itself and the window - 1 keys before it. window >= 1 is a host value, the same
// for every row of the call (KFAMD_EINVAL below 1). Keys below a row's lower bound are excluded as keys at or
// beyond its limit are, by the key index: cache rows that lie outside every row's window may hold NaN (bf16) or
// code 0x7F and NaN scales (FP8). The grid still comes from t_bound (lens is device memory); a workgroup whose
// keys all lie below its rows' windows writes the empty split record and loads no K / V, and the first live one
// starts at the window's first key step (VALU forms) or 64-key tile (MFMA form). window >= t_bound can remove
// no key and launches the kernels of the entry points above: the same bits.
//   kfamd_attn_decode_win_*: kfamd_attn_decode_bf16 / _fp8 (single-row kernel, its stride arrays and workspace).
//   kfamd_attn_extend_win_*, kfamd_attn_chunk_win_*: the signatures of kfamd_attn_extend_gqa_* /
//     kfamd_attn_chunk_gqa_* (G = 1 for plain rows), their stride arrays, row limits, workspaces and split counts.
int kfamd_attn_decode_win_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                               float* lse, void* ws, int B, int H, int D, int t_bound, int window, float scale,
                               const long long* strides, void* stream);
int kfamd_attn_decode_win_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                              const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H, int D,
                              int t_bound, int window, float scale, const long long* strides, void* stream);
int kfamd_attn_extend_win_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                               float* lse, void* ws, int B, int Hkv, int G, int D, int T, int t_bound, int window,
                               float scale, const long long* strides, void* stream);
int kfamd_attn_extend_win_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                              const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int Hkv,
                              int G, int D, int T, int t_bound, int window, float scale, const long long* strides,
                              void* stream);
int kfamd_attn_chunk_win_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                              float* lse, void* ws, int B, int Hkv, int G, int D, int T, int t_bound, int window,
                              float scale, const long long* strides, void* stream);
int kfamd_attn_chunk_win_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                             const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int Hkv,
                             int G, int D, int T, int t_bound, int window, float scale, const long long* strides,
                             void* stream);

// ---- ring-buffer KV cache (attn_kv.hip, attn_kv_mfma.hip, rope_bf16.hip) -------------------------------
// The rule is stated once, in the docstring of kubeflow_rm_amd/ops/decode.py. A ring of capacity cap (a positive
// multiple of 256, KFAMD_EINVAL otherwise) holds key j in slot j % cap, for K, V and the FP8 scales; lens[b] is the
// absolute length and is not bounded by cap; the live keys of row b are max(0, lens[b] - cap) <= j < lens[b].
// Attention: the windowed entry points' signatures with cap in t_bound's place; window >= 1 and
// window + T - 1 <= cap (T = 1 for decode), KFAMD_EINVAL otherwise. The window rule is unchanged. The grid depends on
// (window, T, G, B, H) only: kfamd_attn_ring_nsplit(window, T) = ceil((window + T - 1) / 256) + 1 splits of 256 keys
// (VALU forms) from base_b = (max(lens[b] - T + 1 - window, 0) / 256) * 256 on, rebased per batch row on the device;
// the MFMA form applies its nsplit / split_keys rule to that span (kfamd_attn_chunk_ring_nsplit). The *_ring_workspace
// functions give the bytes of ws for those counts (layouts as for the flat forms). Slots outside every row's window,
// the ones after key lens[b] - 1 included, may hold NaN / 0x7F codes and NaN scales. Positions up to 2^24 are covered.
// Appends: the grouped signatures; position lens[b] + t goes to slot (lens[b] + t) % cap, never dropped; T <= cap.
// The rotary form rotates by the absolute position: the table needs max_pos > the largest lens[b] + T - 1 (the
// caller's check; a position at or beyond max_pos is neither rotated nor stored).
// VGPRs of the RING instantiations (scratch 0 for all): see the tables in attn_kv.hip and attn_kv_mfma.hip.
int kfamd_attn_ring_nsplit(int window, int T);
long long kfamd_attn_decode_ring_workspace(int B, int H, int D, int window);
long long kfamd_attn_extend_ring_workspace(int B, int Hkv, int G, int D, int T, int window);
int kfamd_attn_chunk_ring_nsplit(int B, int Hkv, int G, int T, int window);
long long kfamd_attn_chunk_ring_workspace(int B, int Hkv, int G, int D, int T, int window);
int kfamd_attn_decode_ring_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                                float* lse, void* ws, int B, int H, int D, int cap, int window, float scale,
                                const long long* strides, void* stream);
int kfamd_attn_decode_ring_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                               const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H, int D,
                               int cap, int window, float scale, const long long* strides, void* stream);
int kfamd_attn_extend_ring_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                                float* lse, void* ws, int B, int Hkv, int G, int D, int T, int cap, int window,
                                float scale, const long long* strides, void* stream);
int kfamd_attn_extend_ring_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                               const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int Hkv,
                               int G, int D, int T, int cap, int window, float scale, const long long* strides,
                               void* stream);
int kfamd_attn_chunk_ring_bf16(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                               float* lse, void* ws, int B, int Hkv, int G, int D, int T, int cap, int window,
                               float scale, const long long* strides, void* stream);
int kfamd_attn_chunk_ring_fp8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale,
                              const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int Hkv,
                              int G, int D, int T, int cap, int window, float scale, const long long* strides,
                              void* stream);
int kfamd_kv_append_ring_bf16(const void* qkv, void* k_cache, void* v_cache, const int* pos, int B, int T, int Hq,
                              int Hkv, int D, int cap, long long qb, long long qt, const long long* cache_strides,
                              void* stream);
int kfamd_kv_append_ring_fp8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                             const int* pos, int B, int T, int Hq, int Hkv, int D, int cap, long long qb, long long qt,
                             const long long* cache_strides, void* stream);
int kfamd_kv_append_rope_ring_bf16(void* qkv, void* k_cache, void* v_cache, const int* lens, const float* table,
                                   int max_pos, int B, int T, int Hq, int Hkv, int D, int cap, long long qb,
                                   long long qt, const long long* cache_strides, void* stream);
int kfamd_kv_append_rope_ring_fp8(void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                  const int* lens, const float* table, int max_pos, int B, int T, int Hq, int Hkv,
                                  int D, int cap, long long qb, long long qt, const long long* cache_strides,
                                  void* stream);

// ---- paged KV cache (attn_kv.hip, attn_kv_mfma.hip, rope_bf16.hip) -------------------------------------
// THE PAGE RULE is stated once, in the docstring of kubeflow_rm_amd/ops/decode.py. K, V are page pools
// [n_pages][H][256][D] (FP8: codes, plus scales [n_pages][H][256]); page_table is DEVICE int32 [B][table_stride >=
// ceil(t_bound / 256)] (appends: >= cap / 256), -1 for "no page"; key j of row b lives in page page_table[b][j / 256] at
// row j % 256. The attention entry points take kfamd_attn_decode_* (decode) and kfamd_attn_extend_gqa_* /
// kfamd_attn_chunk_gqa_* (G = 1 for plain rows) with (page_table, table_stride, n_pages) before the stream; the appends
// take kfamd_kv_append_gqa_* / kfamd_kv_append_rope_* the same way, cap (a multiple of 256) in Tcap's place. In every
// stride array the b entries (kb, vb, ksb, vsb) are the PAGE strides. lens, t_bound, lse, the workspaces, split counts
// and return codes are the flat forms'; the split partition, the tile order and the arithmetic are too, so the results
// equal the flat launch's bit for bit on the same contents. Neither a window nor a ring goes with a page table.
// A page id read on the device is used for a load only after clamping into [0, n_pages - 1] (and only for splits /
// tiles that begin below lens[b]), and for a store only if it lies in [0, n_pages): an append drops a position at or
// beyond cap or without a page (the rotary form then leaves the row unrotated). KFAMD_EINVAL also for a null table,
// n_pages < 1, a table narrower than the keys it must cover, cap no multiple of 256.
// VGPRs of the PAGED instantiations (scratch 0 for all): the tables in attn_kv.hip, attn_kv_mfma.hip, rope_bf16.hip.
int kfamd_attn_decode_paged_bf16(const void* q, const void* k_pages, const void* v_pages, const int* lens, void* o,
                                 float* lse, void* ws, int B, int H, int D, int t_bound, float scale,
                                 const long long* strides, const int* page_table, long long table_stride, int n_pages,
                                 void* stream);
int kfamd_attn_decode_paged_fp8(const void* q, const void* k_pages, const void* v_pages, const float* k_scale,
                                const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int H,
                                int D, int t_bound, float scale, const long long* strides, const int* page_table,
                                long long table_stride, int n_pages, void* stream);
int kfamd_attn_extend_paged_bf16(const void* q, const void* k_pages, const void* v_pages, const int* lens, void* o,
                                 float* lse, void* ws, int B, int Hkv, int G, int D, int T, int t_bound, float scale,
                                 const long long* strides, const int* page_table, long long table_stride, int n_pages,
                                 void* stream);
int kfamd_attn_extend_paged_fp8(const void* q, const void* k_pages, const void* v_pages, const float* k_scale,
                                const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int Hkv,
                                int G, int D, int T, int t_bound, float scale, const long long* strides,
                                const int* page_table, long long table_stride, int n_pages, void* stream);
int kfamd_attn_chunk_paged_bf16(const void* q, const void* k_pages, const void* v_pages, const int* lens, void* o,
                                float* lse, void* ws, int B, int Hkv, int G, int D, int T, int t_bound, float scale,
                                const long long* strides, const int* page_table, long long table_stride, int n_pages,
                                void* stream);
int kfamd_attn_chunk_paged_fp8(const void* q, const void* k_pages, const void* v_pages, const float* k_scale,
                               const float* v_scale, const int* lens, void* o, float* lse, void* ws, int B, int Hkv,
                               int G, int D, int T, int t_bound, float scale, const long long* strides,
                               const int* page_table, long long table_stride, int n_pages, void* stream);
int kfamd_kv_append_paged_bf16(const void* qkv, void* k_pages, void* v_pages, const int* pos, int B, int T, int Hq,
                               int Hkv, int D, int cap, long long qb, long long qt, const long long* cache_strides,
                               const int* page_table, long long table_stride, int n_pages, void* stream);
int kfamd_kv_append_paged_fp8(const void* qkv, void* k_pages, void* v_pages, float* k_scale, float* v_scale,
                              const int* pos, int B, int T, int Hq, int Hkv, int D, int cap, long long qb, long long qt,
                              const long long* cache_strides, const int* page_table, long long table_stride,
                              int n_pages, void* stream);
int kfamd_kv_append_rope_paged_bf16(void* qkv, void* k_pages, void* v_pages, const int* lens, const float* table,
                                    int max_pos, int B, int T, int Hq, int Hkv, int D, int cap, long long qb,
                                    long long qt, const long long* cache_strides, const int* page_table,
                                    long long table_stride, int n_pages, void* stream);
int kfamd_kv_append_rope_paged_fp8(void* qkv, void* k_pages, void* v_pages, float* k_scale, float* v_scale,
                                   const int* lens, const float* table, int max_pos, int B, int T, int Hq, int Hkv,
                                   int D, int cap, long long qb, long long qt, const long long* cache_strides,
                                   const int* page_table, long long table_stride, int n_pages, void* stream);

// ---- rotary position embeddings (rope_bf16.hip)-----------------------------------------------------
// table: fp32 [max_pos][D] contiguous, row p = cos(p f_i) | sin(p f_i), i < D/2 (built on the host). The
// rotation is rotate-half: y[i] = x[i] c - x[i + D/2] s, y[i + D/2] = x[i + D/2] c + x[i] s, in fp32 without
// FMA contraction, rounded once to bf16. The activation is [B][T][(Hq + 2 Hkv) D], q | k | v (element strides
// qb, qt); D = 64 / 128.
// kfamd_rope_qkv_bf16: rotates the q and k head rows IN PLACE, v untouched. Row (b, t) is at position
//   (pos ? pos[b] : 0) + t (pos: device int32 [B] or null); a row at or beyond max_pos is left as it is.
//   inverse != 0: the inverse rotation (s -> -s), the backward of the forward map.
// kfamd_kv_append_rope_bf16 / _fp8: kfamd_kv_append_gqa_bf16 / _fp8 of a rotary layer in one launch: position
//   lens[b] + t, q and k rotated in place, the rotated K row and the V row written to cache row lens[b] + t
//   (FP8: the bf16-rounded rotated K is what is quantised). Rows at or beyond Tcap are neither appended nor
//   rotated. KFAMD_EINVAL also for max_pos < Tcap. Hq / Hkv in {1, 2, 4, 8, 16}.
// KFAMD_EALIGN: the activation, the caches or the table not 16-B aligned.
int kfamd_rope_qkv_bf16(void* qkv, const float* table, const int* pos, int max_pos, int B, int T, int Hq, int Hkv, int D,
                        long long qb, long long qt, int inverse, void* stream);
int kfamd_kv_append_rope_bf16(void* qkv, void* k_cache, void* v_cache, const int* lens, const float* table, int max_pos,
                              int B, int T, int Hq, int Hkv, int D, int Tcap, long long qb, long long qt,
                              const long long* cache_strides, void* stream);
int kfamd_kv_append_rope_fp8(void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale, const int* lens,
                             const float* table, int max_pos, int B, int T, int Hq, int Hkv, int D, int Tcap,
                             long long qb, long long qt, const long long* cache_strides, void* stream);

// Weight-streaming NT GEMM for 1 <= M <= 16 (gemm_skinny_bf16.hip): C[M][N] = act(alpha * A[M][K] .
// W[N][K]^T + bias[N]) (+ R[M][N]); K % 8 == 0, A / W rows 16-B aligned, any N, epilogue semantics of
// kfamd_gemm_nt_bf16. KFAMD_EINVAL: M outside 1..16 (or K % 8); KFAMD_EALIGN: alignment.
int kfamd_gemm_nt_skinny_bf16(const void* A, const void* W, void* C, const void* bias, const void* R, int M, int N,
                              int K, long long lda, long long ldw, long long ldc, long long ldr, float alpha, int act,
                              void* stream);
// the same with the arithmetic pattern forced (tests / bench): 0 = by M, 1 = VALU (M <= 8), 2 = MFMA
int kfamd_gemm_nt_skinny_bf16_path(int path, const void* A, const void* W, void* C, const void* bias, const void* R,
                                   int M, int N, int K, long long lda, long long ldw, long long ldc, long long ldr,
                                   float alpha, int act, void* stream);

// The same on 8-bit weights, W8A16 (gemm_skinny_w8.hip): C[M][N] = act(alpha * wscale[n] * (A[M][K] .
// codes[N][K]^T) + bias[n]) (+ R[M][N]). codes: OCP e4m3fn bytes, row stride ldw BYTES; wscale: fp32 [N],
// contiguous, required (the format of the FP8 KV cache's rows). K >= 16, K % 16 == 0, codes 16-B aligned,
// ldw % 16 == 0, A as above. NaN codes (0x7F, 0xFF) are out of contract. Return codes and path as the
// bf16 kernel's.
int kfamd_gemm_nt_skinny_w8(const void* A, const void* codes, const float* wscale, void* C, const void* bias,
                            const void* R, int M, int N, int K, long long lda, long long ldw, long long ldc,
                            long long ldr, float alpha, int act, void* stream);
int kfamd_gemm_nt_skinny_w8_path(int path, const void* A, const void* codes, const float* wscale, void* C,
                                 const void* bias, const void* R, int M, int N, int K, long long lda, long long ldw,
                                 long long ldc, long long ldr, float alpha, int act, void* stream);
// bench only: also forces the MFMA form's 8-row tiles per workgroup (1, 2, 4) or the VALU form's weight
// rows per wave (2, 4); tiles = 0 selects by N as the other two entry points do
int kfamd_gemm_nt_skinny_w8_tiles(int path, int tiles, const void* A, const void* codes, const float* wscale,
                                  void* C, const void* bias, const void* R, int M, int N, int K, long long lda,
                                  long long ldw, long long ldc, long long ldr, float alpha, int act, void* stream);

// ---- SwiGLU (the rule: kubeflow_rm_amd/ops/swiglu.py) ------------------------------------------------
// A gated up-projection weight is W [N = 2F][K] with INTERLEAVED rows: row 2j is gate j, row 2j + 1 is up j
// (bias [2F] and, on 8-bit weights, wscale [2F] in the same order). With z = alpha * A . W^T + bias (8-bit:
// alpha * wscale[n] * (A . codes^T) + bias[n], the scale before the bias as above), the output is
//   C[m][j] = silu(z[m][2j]) * z[m][2j + 1],  silu(v) = v / (1 + exp(-v)),  fp32, rounded once to bf16.
// Gated weight-streaming GEMM, 1 <= M <= 16 (gemm_skinny_bf16.hip / gemm_skinny_w8.hip with GLU): C [M][F],
// ldc >= F. No activation code and no residual. N is the WEIGHT's row count 2F and must be even (KFAMD_EINVAL);
// the other shape / alignment rules, return codes, `path` (0 = by M and N, 1 = VALU with M <= 8, 2 = MFMA) and
// `tiles` (0 = by N, else the MFMA form's 8-row tiles per workgroup 1 / 2 / 4 = 4 / 8 / 16 pairs, or the VALU
// form's weight rows per wave 2 / 4 = 1 / 2 pairs) are the ungated kernels'.
int kfamd_gemm_nt_skinny_bf16_glu(const void* A, const void* W, void* C, const void* bias, int M, int N, int K,
                                  long long lda, long long ldw, long long ldc, float alpha, void* stream);
int kfamd_gemm_nt_skinny_bf16_glu_path(int path, const void* A, const void* W, void* C, const void* bias, int M, int N,
                                       int K, long long lda, long long ldw, long long ldc, float alpha, void* stream);
int kfamd_gemm_nt_skinny_bf16_glu_tiles(int path, int tiles, const void* A, const void* W, void* C, const void* bias,
                                        int M, int N, int K, long long lda, long long ldw, long long ldc, float alpha,
                                        void* stream);
int kfamd_gemm_nt_skinny_w8_glu(const void* A, const void* codes, const float* wscale, void* C, const void* bias, int M,
                                int N, int K, long long lda, long long ldw, long long ldc, float alpha, void* stream);
int kfamd_gemm_nt_skinny_w8_glu_path(int path, const void* A, const void* codes, const float* wscale, void* C,
                                     const void* bias, int M, int N, int K, long long lda, long long ldw, long long ldc,
                                     float alpha, void* stream);
int kfamd_gemm_nt_skinny_w8_glu_tiles(int path, int tiles, const void* A, const void* codes, const float* wscale,
                                      void* C, const void* bias, int M, int N, int K, long long lda, long long ldw,
                                      long long ldc, float alpha, void* stream);
// The gate as its own pass (swiglu_bf16.hip), any row count: z [rows][2F] (row stride ldz >= 2F) -> h [rows][F]
// (ldh >= F); backward dh [rows][F] (lddh), z -> dz [rows][2F] (lddz): dz[2j] = dh u s (1 + g (1 - s)),
// dz[2j + 1] = dh silu(g), s = 1 / (1 + exp(-g)). 16-B loads and stores when F % 8 == 0, every stride % 8 == 0
// and the bases are 16-B aligned; a scalar path otherwise (never KFAMD_EALIGN). Padding between rows is not touched.
int kfamd_swiglu_fwd_bf16(const void* z, void* h, long long rows, int F, long long ldz, long long ldh, void* stream);
int kfamd_swiglu_bwd_bf16(const void* dh, const void* z, void* dz, long long rows, int F, long long lddh, long long ldz,
                          long long lddz, void* stream);

// RMSNorm backward (layernorm_bf16.hip, the LayerNorm backward's kernels with mean = 0, no c2 term, no dbeta):
// dx = rstd * (gamma dy - xhat * mean(gamma dy xhat)) (+ dres, optional, not aliasing dx), dgamma = column sums of
// dy * xhat (fp32, or bf16 when dgb_bf16; optional), xhat = x * rstd, rstd from kfamd_rmsnorm_fwd_bf16. workspace:
// kfamd_layernorm_bwd_workspace bytes (required with dgamma).
int kfamd_rmsnorm_bwd_bf16(const void* dy, const void* dres, const void* x, const void* gamma, const float* rstd,
                           void* dx, void* dgamma, int dgb_bf16, float* workspace, int rows, int hidden, void* stream);
// kfamd_layernorm_bwd_bf16_v3 / kfamd_rmsnorm_bwd_bf16 (rms != 0: mean and dbeta are ignored) with the launch path
// forced (tests / bench), whatever KFAMD_LN_BWD_SPLIT says:
//   path 0: the launcher's rule   1: fused dx + column partials in one pass (dgamma or dbeta given; hidden 512 *
//   {1,2,3,4} on 16-B pointers, 256 * {1,3,5} on 8-B pointers)   2: dx wave per row (the forward's widths and
//   alignment), then the column partials   3: dx one workgroup per row (any hidden, any alignment), then the partials
// A path the shape or the alignment cannot take, or outside 0 .. 3: KFAMD_EINVAL, nothing launched.
int kfamd_norm_bwd_bf16_path(int rms, int path, const void* dy, const void* dres, const void* x, const void* gamma,
                             const float* mean, const float* rstd, void* dx, void* dgamma, void* dbeta, int dgb_bf16,
                             float* workspace, int rows, int hidden, void* stream);

// Token sampling (sample_bf16.hip): one token per row of bf16 logits [B][V] (row stride ld elements, the
// vocabulary contiguous, 2-byte alignment only; 1 <= V <= 2^20; -inf allowed, NaN / an all -inf row out of
// contract). Tokens are ordered by logit descending, equal logits by index ascending.
//   inv_temp == 0 or top_k == 1: the first token of that order (u is not read).
//   otherwise w_i = exp((x_i - x_max) * inv_temp); top_k (0 = none) keeps the first min(top_k, V) tokens of
//   the order; top_p (1 = none) then keeps the shortest prefix whose mass reaches top_p * (mass of the
//   top-k set), at least one token; the result is the first kept token in INDEX order whose inclusive
//   running sum of kept weights exceeds u * W (W: the kept mass).
// u: fp32 [S][B]; step: device int32 selecting the row u[*step] (nullptr: row 0; a *step outside [0, S)
// makes the launch write nothing). out: int64 [B]. seq (optional): int64 [B][seq_ld >= S], column *step
// is written. stop_token >= 0 with done (int32 [B], required then): a row whose flag is set emits
// stop_token; any other row emits its token and sets its flag when the token is stop_token. stop_token
// < 0: no stop (done must be nullptr). Everything a step needs is read from device memory, so a captured
// launch replays while *step advances; the kernel never advances it.
int kfamd_sample_bf16(const void* logits, long long ld, const float* u, const int* step, long long* out,
                      long long* seq, long long seq_ld, int* done, int B, int V, int S, float inv_temp, int top_k,
                      float top_p, long long stop_token, void* stream);

#ifdef __cplusplus
}
#endif
