/*
 * gear_hip.h -- C ABI of libgear_hip.so: the MI355X (gfx950) KV-cache compress / decompress hot path.
 *
 * This is the drop-in boundary.  The reference exposes this path through Python
 * functions backed by Triton kernels and one pybind11 CUDA extension (`kivi_gemv`,
 * cuda_supported_gear/quant/csrc/pybind.cpp:5-8, gemv_cuda.h:13-21) that take torch::Tensor -- i.e. it has
 * no C ABI of its own.  Each entry point below names the reference interface it replaces; the Python
 * mirror of the reference's operator API (gear_amd/quant/new_pack.py, gear_amd/quant/matmul.py, ...) binds
 * these symbols with ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated otherwise; buffers are caller-allocated, contiguous,
 *     16-byte aligned; nothing here allocates or synchronises;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - return value: 0 = ok, < 0 = error (argument check or launch failure); gear_last_error() returns a
 *     thread-local message for the last failing call;
 *   - fp16 tensors are IEEE binary16; "mode" selects the arithmetic:
 *       GEAR_MODE_FP16_STEPWISE (0): torch-eager fp16 semantics of cuda_supported_gear/quant/new_pack.py
 *                                    (:237-240, :273-278) -- packed payload bit-exact; scale/mn are fp16;
 *       GEAR_MODE_FP32          (1): the simulated path's fp32 arithmetic
 *                                    (GenerationBench/.../Simulated/compress_function.py:14-33, :116-125);
 *                                    scale/mn are float32;
 *   - bits in {2,4} (8 also accepted by the quantizers), fpi = 32/bits codes per int32 word, LSB first
 *     (new_pack.py:104, :148-153).
 */
#ifndef GEAR_HIP_H
#define GEAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEAR_MODE_FP16_STEPWISE 0
#define GEAR_MODE_FP32 1

#define GEAR_DTYPE_F16 0
#define GEAR_DTYPE_F32 1

/* Library / build identification. */
const char* gear_last_error(void);
int gear_abi_version(void);
/* Run-time options: switches that select an alternative, equally exact code path (used by the tests to reach the
 * paths ordinary inputs do not).  Names: "attn_generic", "lowrank_generic", "rows_hist_only", "rows_wg_only", "rows_v1", "rows_masked",
 * "kfused_generic", "kselect_slow", "kfused_no_tr", "gram_fused", "gram_nstg", "decomp_general", "decomp_rpb", "kfused_nslab", "attn_fold" (decode attention: 1 = the merge of the partial results inside the partial launch; off by default, measured
 * no faster), "kfused_main" (1 = k_main_kernel instead of k_dense_kernel for fp32 arithmetic), "kfused_eout" (1 = k_dense_kernel writes the error matrix, the Q pass reads it), "kfused_one" (the
 * single-read K kernel, csrc/kone.hip: 1 = wherever it applies; off by default -- measured slower than the chain), and for the decode
 * attention "attn_gqa_group" (one workgroup per KV head serves its 2 / 4 / 8 query heads), "attn_win_chunk" (fp16 window as one more
 * chunk of the split: 0 = on the vector short-chunk kernel, 1 = always, -1 = never), "attn_keep_chunk_index", "attn_mfma" (the matrix-core variant of the short-chunk kernel: 0 = for grouped-query
 * shapes, 1 = always, -1 = never) -- measured alternatives of round 5, all off / automatic by default (gear_amd/csrc/common.h says
 * what each measured).  Each is also read once from the environment (GEAR_<NAME>) when the library is first used.  Returns 0, or -1
 * for an unknown name. */
int gear_set_option(const char* name, int value);

/* ---- a1 / a2 / a3(V): group quantize + bit-pack along the last dim ------------------------------------
 * Replaces triton_quantize_and_pack_along_last_dim (cuda_supported_gear/quant/new_pack.py:217-250),
 * ..._witherror (:253-288, with ALL columns packed -- reference defect B1) and quant_and_pack_vcache (:30-48).
 *   x     : fp16 [rows, L]           code : int32 [rows, L/fpi]
 *   scale, mn : [rows, L/group]  fp16 (mode 0) / float32 (mode 1)
 *   err   : optional fp16 [rows, L] = x - dequant (mode 0: fp16-stepwise, new_pack.py:277-278;
 *           mode 1: fp16(x - fp16(dequant))), NULL to skip.
 * Requires L % group == 0, group a power of two in [16, 1024], L % 16 == 0.
 * Zero-range groups (reference: NaN, defect B6) produce code 0, scale 0.
 */
int gear_quant_pack_lastdim(const void* x, int64_t rows, int L, int group, int bits, int mode, void* code,
                            void* scale, void* mn, void* err, void* stream);

/* ---- a3(K): token-major K tile, groups of `group` consecutive tokens per channel, packed along T --------
 * Replaces quant_and_pack_kcache (new_pack.py:8-27).
 *   x : fp16 [bh, T, D]   code : int32 [bh, T/fpi, D]   scale, mn : [bh, T/group, D]   err : optional fp16 [bh, T, D]
 * Requires D % 8 == 0, T % group == 0, group % fpi == 0.
 */
int gear_quant_pack_k(const void* x, int64_t bh, int T, int D, int group, int bits, int mode, void* code, void* scale,
                      void* mn, void* err, void* stream);

/* ---- a3: unpack + dequantize to fp16 -----------------------------------------------------------------------
 * Replace unpack_and_dequant_vcache (new_pack.py:69-83) and unpack_and_dequant_kcache (:51-66).
 */
int gear_unpack_dequant_lastdim(const void* code, const void* scale, const void* mn, int64_t rows, int L, int group,
                                int bits, int mode, void* out, void* stream);
int gear_unpack_dequant_k(const void* code, const void* scale, const void* mn, int64_t bh, int T, int D, int group,
                          int bits, int mode, void* out, void* stream);

/* ---- a6: decompress-into-attention GEMV ("outer dim" layout) ---------------------------------------------
 * Replaces kivi_gemv.gemv_forward_cuda_outer_dim (gemv_cuda.cu:518-564; kernels :264-434) AND the
 * transpose().contiguous() re-layout that cuda_bmm_fA_qB_outer performs on every call
 * (cuda_supported_gear/quant/matmul.py:205, :215-216): this entry point consumes the layout the Python
 * operator receives.
 *   out[ba, n] = sum_k a[ba, k] * (scale[bw, k, n/group] * code[bw, k, n] + zero[bw, k, n/group]),  bw = ba / n_rep
 *   a    : fp16 [BA, K]                     qB : int32 [BW, K, N/fpi]   (BW = BA / n_rep)
 *   scale, zero : [BW, K, N/group]          out : fp16 [BA, N]
 *   ldq / lds: row pitch (in int32 words / in scale elements) of qB and scale/zero rows; pass 0 for dense.
 *   n_rep : query heads per KV head (1 = MHA; the reference's `mqa` flag, gemv_cuda.cu:276-279).
 *   workspace: device scratch of at least gear_gemv_outer_workspace(...) bytes (split-K partial sums).
 * fp32 accumulation, one fp16 rounding at the end (gemv_cuda.cu:343-345).  bits in {2,4}; group % fpi == 0.
 */
size_t gear_gemv_outer_workspace(int64_t BA, int K, int N, int bits);
int gear_gemv_outer(const void* a, const void* qB, const void* scale, const void* zero, int64_t BA, int n_rep, int K,
                    int N, int group, int bits, int mode, int64_t ldq, int64_t lds, void* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* The same GEMV on the reference extension's OWN argument layout -- K innermost, what cuda_bmm_fA_qB_outer produces with its
 * per-call transpose(1, 2).contiguous() (matmul.py:205, :215-216) and hands to kivi_gemv.gemv_forward_cuda_outer_dim
 * (gemv_cuda.h:13-21: _in_feats, _kernel, _scaling_factors, _zeros, bit, group_size, nh, mqa):
 *   in_feats fp16 [BA, K]      kernel int32 [BW, N / fpi, K]      scaling_factors, zeros [BW, N / group, K]      out fp16 [BA, N]
 *   n_rep = 1 (one kernel row block per query head), nh with mqa, or any divisor of the query heads (GQA).
 * For a maintainer who keeps matmul.py line by line and swaps only the extension call; gear_gemv_outer (above) is the entry that
 * makes the re-layout unnecessary.  Same arithmetic, no workspace. */
int gear_gemv_outer_dim(const void* in_feats, const void* kernel, const void* scaling_factors, const void* zeros, int64_t BA,
                        int n_rep, int K, int N, int group, int bits, int mode, void* out, void* stream);

/* ---- a7: dequant GEMV + low-rank correction in two launches -------------------------------------------------------------
 * Replaces matmul_withlrap (cuda_supported_gear/modeling_llamagear.py:54-111): cuda_bmm_fA_qB_outer followed by ~8 eager matmul /
 * permute / slice-assign launches for the prefill factors (pbase[0], qbase[0]) and the per-block factors stacked on a leading
 * dim (pbase[1], qbase[1], :71-85 / :87-108).  The GEMV kernel of gear_gemv_outer writes fp32 partial sums; ONE epilogue kernel
 * reduces them, adds the low-rank terms in fp32 and rounds to fp16 once.
 *   kind 0 "key":   K = head_dim, N = Tp + nbuf * blk tokens;  P0 [BW, Tp, r], Q0 [BW, K, r];  P1 [nbuf, BW, blk, r], Q1 [nbuf, BW, K, r]
 *   kind 1 "value": K = Tp + nbuf * blk tokens, N = head_dim;  P0 [BW, N, r], Q0 [BW, Tp, r];  P1 [nbuf, BW, N, r], Q1 [nbuf, BW, blk, r]
 *   (BW = BA / n_rep KV heads; all factors fp16; nbuf == 0: prefill factors only; dense row pitches.) */
size_t gear_gemv_outer_lrap_workspace(int64_t BA, int K, int N, int bits);
int gear_gemv_outer_lrap(const void* a, const void* qB, const void* scale, const void* zero, int64_t BA, int n_rep, int K, int N,
                         int group, int bits, int mode, int kind, const void* P0, const void* Q0, int Tp, const void* P1,
                         const void* Q1, int nbuf, int blk, int r, void* out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- a11 (+ a9): one pass per row -- outlier top-k select, mean fill, group quantize, pack, error -------------
 * Replaces gears_channelQ / gears_tokenQ (GenerationBench/.../Simulated/compress_function.py:261-333) and, with
 * k == 0, the fake_groupwise_*_asymmetric_quantization functions (:7-67, :100-160), producing a REAL payload.
 * A row is the unit of outlier selection: a token across all heads (V: nseg = H segments of D) or a channel
 * across all tokens (K in the K^T layout [B,H,D,T]: one segment of T).
 *   row r starts at element (r / rows_inner) * outer_stride + (r % rows_inner) * inner_stride; its element j
 *   lives at + (j / seglen) * seg_stride + j % seglen.          len = nseg * seglen <= 16384.
 *   x fp16; code/scale/mn/err use the same geometry with the last dim divided by fpi / group / 1.
 *   k  : outliers per side per row (compress_function.py:265-267 / :300-303); 0 disables the sparse part.
 *   oidx uint16 [n_rows, 2k] (index within the row; first k = the k smallest, then the k largest, each sorted by
 *   index), oval fp16 [n_rows, 2k] (original values), omean float [n_rows] (optional).  Ties across the selection
 *   boundary: lower index first (torch.topk leaves it implementation-defined).
 *   err: optional fp16, x - fp16(dequant) with 0 at outlier positions.
 */
int gear_compress_rows(const void* x, int64_t n_rows, int rows_inner, int64_t outer_stride, int64_t inner_stride,
                       int nseg, int seglen, int64_t seg_stride, int group, int bits, int mode, int k, void* code,
                       void* scale, void* mn, void* err, void* oidx, void* oval, void* omean, void* stream);

/* ---- a5 / a11 (K side) fused: token-major K -> complete K payload, no transpose, no K^T intermediates ------------------
 * Replaces, for head_dim 128, the chain  key.transpose(2, 3).contiguous()  (cuda_supported_gear/modeling_llamagear.py:268,
 * :403) -> gears_channelQ (GenerationBench/.../Simulated/compress_function.py:261-296) -> fake_poweriteration_group
 * (:69-98) / key_compression (modeling_llamagear.py:23-38):  per-channel outlier selection over the T tokens, mean fill,
 * group quantization along T, bit-packing into the channel-major K^T payload layout, the fp16 error and its rank-r
 * power iteration -- in four launches (select, fused quantize + pack + Gram on the matrix cores, per-head solve, Q pass)
 * that read x three times and never write the error matrix: the Q pass rebuilds E = x - dequant from x, the stored codes /
 * scale / mn and the outlier bitmap (the round-1 chain moved 12.6 bytes per element through HBM, this 6.9).
 *   x     fp16 [BH, T, 128] token-major                       T % 64 == 0, 64 <= T <= 16384; group in {32, 64}; bits in {2, 4}
 *   code  int32 [BH, 128, ldc]   words  t_off / fpi ..  of every channel row are written (ldc = row pitch in words)
 *   scale, mn [BH, 128, lds]     fp16 (mode 0) / float (mode 1), groups t_off / group ..
 *   k     outliers per side per channel row (0: none).  oidx / oval uint16 / fp16 [BH, 128, 2, kcap]: side slot 0 = the k
 *         smallest, slot 1 = the k largest, each ascending by token, written at list position o_off ..; the stored token
 *         index is t_off + t.  Ties at the selection boundary: lower token first (as gear_compress_rows).
 *   rank  0: no low-rank part.  P0 float [BH, 128, rank]; P_out fp16, head bh at element offset
 *         (bh / p_inner) * p_outer_stride + (bh % p_inner) * 128 * rank;  Q_out fp16 [BH, q_tcap, rank], rows q_toff ..
 *   variant: bit 0 = element-by-element tile arithmetic, bit 1 = always the exact slow selection, bit 2 = 16-bit LDS reads
 *         instead of the transposing ones for the matrix-core operands (cross-checks); measurement hooks (bench.py times
 *         the kernels of the chain one by one with them): bit 3 = reuse the selection a previous identical call left in the
 *         workspace, bit 4 = return after the fused quantize + Gram kernel, bit 5 = return after the selection
 *   workspace: gear_compress_key_fused_workspace(BH, T, k, rank) bytes of device scratch.
 * With t_off / ldc / lds / q_tcap / kcap the call appends a block to a pre-allocated streaming cache in place.
 */
size_t gear_compress_key_fused_workspace(int64_t BH, int T, int k, int rank);
int gear_compress_key_fused(const void* x, int64_t BH, int T, int group, int bits, int mode, int k, void* code, void* scale,
                            void* mn, int64_t ldc, int64_t lds, int t_off, int rank, int loop, const void* P0, void* P_out,
                            int64_t p_inner, int64_t p_outer_stride, void* Q_out, int q_tcap, int q_toff, void* oidx,
                            void* oval, int kcap, int o_off, int variant, void* workspace, size_t workspace_bytes,
                            void* stream);

/* V side, written in place (the streaming cache): V [B, H, T, 128] token-major -> payload rows t_off .. t_off + T of tensors
 * with `tcap` token rows per head: code int32 [B, H, tcap, 128/fpi], scale / mn [B, H, tcap, 128/group], sparse lists
 * oidx / oval [B, tcap, 2k] (gears_tokenQ semantics: a row = one token across the H heads,
 * GenerationBench/.../Simulated/compress_function.py:297-333), factors as gear_compress_key_fused.  The row compressor with an
 * output geometry, then the Gram-matrix power iteration and the Q pass. */
size_t gear_compress_value_fused_workspace(int64_t B, int H, int T, int rank);
int gear_compress_value_fused(const void* x, int64_t B, int H, int T, int group, int bits, int mode, int k, void* code,
                              void* scale, void* mn, int tcap, int t_off, int rank, int loop, const void* P0, void* P_out,
                              int64_t p_inner, int64_t p_outer_stride, void* Q_out, int q_tcap, int q_toff, void* oidx,
                              void* oval, void* workspace, size_t workspace_bytes, void* stream);

/* ---- head-sharded V rows: the outlier selection of a row that spans the heads of several GPUs ------------------------------
 * gears_tokenQ selects the k smallest and k largest values of a token's row over ALL heads (compress_function.py:297-333, two
 * torch.topk over H * D columns) and fills them with the row mean.  With the heads spread over `world` ranks:
 *   gear_vsel_candidates   this rank's part of every row (same row geometry as gear_compress_rows: n_rows rows of nseg segments of
 *                          seglen contiguous fp16 elements) -> cand uint32 [n_rows][2k + 2]: per side its k best elements as global
 *                          composites (16-bit order key << 16 | 0xFFFF - global column: ties -> lower column), then the exact
 *                          fp64 sum of the local part (bit pattern, two words).  col0 = global column of the rank's first element;
 *                          a full row has at most 65535 elements.
 *   (the ranks all-gather cand -> cand_all [world][n_rows][2k + 2]; 4 (2k + 2) bytes per row and rank)
 *   gear_vsel_thresholds   -> thr uint32 [n_rows][2] (the k-th largest composite, large side then small side), fill float [n_rows]
 *                          (mean of the full row of row_len_total elements; mode 0: rounded to fp16 like the row kernels' fill)
 *   gear_compress_value_sharded = gear_compress_value_fused with that selection instead of its own: a rank stores the outliers
 *                          that fall into its heads (0 .. k per side and row; unused list slots: index 0xFFFF, value 0).
 * The concatenated shard payloads are the unsharded payload (mode 0: bit for bit; mode 1: the unsharded kernel's fill is an fp32
 * tree sum, here it is the correctly rounded mean -- the last place of the fill can differ, the selection cannot).
 * The reference has no multi-GPU path; this keeps its single-GPU semantics under head sharding.
 * Range of the "shard payloads == unsharded payload, bit for bit" guarantee: |x| < 2^12 -- there the fp64 row sums behind the fill
 * value are exact and hence independent of how the row is split; larger magnitudes can move a fill by one unit in the last place.
 */
int gear_vsel_candidates(const void* x, int64_t n_rows, int rows_inner, int64_t outer_stride, int64_t inner_stride, int nseg,
                         int seglen, int64_t seg_stride, int k, int col0, void* cand, void* stream);
int gear_vsel_thresholds(const void* cand_all, int world, int64_t n_rows, int k, int64_t row_len_total, int mode, void* thr,
                         void* fill, void* stream);
int gear_compress_value_sharded(const void* x, int64_t B, int H, int T, int group, int bits, int mode, int k, void* code, void* scale,
                                void* mn, int tcap, int t_off, int rank, int loop, const void* P0, void* P_out, int64_t p_inner,
                                int64_t p_outer_stride, void* Q_out, int q_tcap, int q_toff, void* oidx, void* oval, int col0,
                                const void* thr, const void* fill, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a12 (KCVT variants): ONE quantization group per row -------------------------------------------------------------
 * Replaces fake_groupwise_channel_asymmetric_quantization_new(key, bits, seq_len) and
 * fake_groupwise_token_asymmetric_quantization(value, bits, num_head * sep_dim) of the KCVT / GEAR-KCVT / GEARL-KCVT branches
 * (GenerationBench/.../Simulated/compress_function.py:441-452, :496-525, :555-582), optionally around the row's sparse outliers
 * (gears_channelQ / gears_tokenQ with that group size).  Geometry as gear_compress_rows; len = nseg * seglen <= 16384, any
 * length.  oidx: uint16 [n_rows, 2k] as gear_compress_rows writes it (k == 0: none).
 *   y   fp16, same geometry: quantize -> dequantize, outliers keep their original value
 *   err optional fp16 x - y (0 at the outliers)
 */
int gear_quant_rows_whole(const void* x, int64_t n_rows, int rows_inner, int64_t outer_stride, int64_t inner_stride, int nseg,
                          int seglen, int64_t seg_stride, int bits, int mode, const void* oidx, int k, void* y, void* err,
                          void* stream);

/* ---- a11 / a12 with a sequence length that is not a multiple of the group ------------------------------------------------
 * gears_channelQ / gears_tokenQ (GenerationBench/.../Simulated/compress_function.py:261-333) on rows of ANY length: the k
 * smallest / k largest of the WHOLE row are selected inside the kernel (ties: lower index first) and replaced by the whole
 * row's mean for the quantization; fake_groupwise_channel_asymmetric_quantization_cluster then quantizes the first
 * floor(len / group) * group elements in groups of `group` consecutive elements and leaves the tail untouched (:107-122).
 * Geometry as gear_compress_rows; len = nseg * seglen <= 16384, at most 2048 groups per row, 2k <= len.
 *   y   fp16, same geometry: quantize -> dequantize of the prefix, outliers and tail keep their original value
 *   err optional fp16 x - y (0 at the outliers and in the tail)
 */
int gear_quant_rows_ragged(const void* x, int64_t n_rows, int rows_inner, int64_t outer_stride, int64_t inner_stride, int nseg,
                           int seglen, int64_t seg_stride, int group, int bits, int mode, int k, void* y, void* err,
                           void* stream);

/* ---- a4 / a10: low-rank power iteration ---------------------------------------------------------------------
 * Replaces headwise_lrap (cuda_supported_gear/quant/new_pack.py:291-311) and fake_poweriteration_group
 * (compress_function.py:69-98).  for i < loop: [last: P = orth(P)] Q = E P [last: Q = orth(Q)] P = E^T Q.
 *   E  : [bh, S, Dm] (transposed == 0) or its transpose [bh, Dm, S] (transposed == 1); fp16 or float32
 *   P0 : float32 [bh, Dm, r] initial basis (the reference draws it with torch.rand on the CPU generator; the
 *        caller supplies it so that runs are reproducible);   P_out [bh, Dm, r], Q_out [bh, S, r] fp16 / float32.
 *   1 <= r <= 16.  Per-(batch, head) bases (reference defect B3 not reproduced).
 */
size_t gear_lowrank_workspace(int64_t bh, int S, int Dm, int r);
int gear_lowrank(const void* E, int e_dtype, int transposed, int64_t bh, int S, int Dm, int r, int loop,
                 const void* P0, void* P_out, void* Q_out, int out_dtype, void* workspace, size_t workspace_bytes,
                 void* stream);

/* ---- decompress to fp16: dequant + low-rank + sparse restore ------------------------------------------------
 * out = fp16(fp16(dequant) + Q P^T), outliers restored from their stored fp16 value (compress_function.py:204-220
 * assembles the simulated result the same way).  Geometry as gear_compress_rows.
 *   kind 0: V rows (row = (b, t), rows_inner = T, nseg = H, seglen = D)   kind 1: K^T rows (row = (bh, d),
 *   rows_inner = D, one segment of T).  P fp16 [BH, D, r], Q fp16 [BH, T, r] (r == 0: none).
 * Limits (GEAR_ERR_ARG otherwise): the rows of one outer index must span fewer than 2^31 elements (the kernel adds 32-bit lane
 * offsets to a 64-bit base per workgroup), strides multiples of the group size.
 */
int gear_decompress_rows(const void* code, const void* scale, const void* mn, int64_t n_rows, int rows_inner,
                         int64_t outer_stride, int64_t inner_stride, int nseg, int seglen, int64_t seg_stride, int group,
                         int bits, int mode, int kind, const void* P, const void* Q, int r, int T, int D,
                         const void* oidx, const void* oval, int k, void* out, void* stream);

/* ---- batched fp16 transpose [bh, R, C] -> [bh, C, R] ------------------------------------------------------------
 * Replaces the caller-side key_states.transpose(2, 3).contiguous() of the attention hook
 * (cuda_supported_gear/modeling_llamagear.py:268, :403).  R, C multiples of 8.
 */
int gear_transpose_f16(const void* x, int64_t bh, int R, int C, void* y, void* stream);

/* ---- a6 + a7 (+ outliers): single-token decode attention over the compressed cache ---------------------------
 * One pass over the packed bytes replaces cuda_bmm_fA_qB_outer for K and V (cuda_supported_gear/quant/matmul.py:178),
 * the low-rank bmm chains of matmul_withlrap (modeling_llamagear.py:64-108), the fp32 softmax (:313) and the merge with
 * the fp16 residual window (:256-261, :329-333); also applies the sparse outlier term (not stored by the reference's
 * fused path).  head_dim must be 128.
 *   q      fp16 [B, Hq, 128]
 *   K payload (channel-major, as gear_compress_rows produces for K^T): kcode int32 [B*Hkv, 128, ldk], kscale / kmn
 *     [B*Hkv, 128, lsk], kP fp16 [B*Hkv, 128, rk] (channel side), kQ fp16 [B*Hkv, tf_k, rk] (token side),
 *     koidx / koval uint16 / fp16 [B*Hkv, 128, 2*kk] (token index, each half ascending) -- factors / outliers may be NULL
 *   V payload (token-major): vcode int32 [B*Hkv, tcap_v, 128/fpi], vscale / vmn [B*Hkv, tcap_v, 128/group], vP fp16
 *     [B*Hkv, 128, rv], vQ fp16 [B*Hkv, tf_v, rv], voidx / voval [B, tcap_v, 2*kv] (column Hkv-head*128 + d)
 *   kwin / vwin fp16 [B*Hkv, W, 128]: the W <= 128 most recent, still uncompressed tokens (NULL when W == 0)
 *   T compressed tokens (multiple of fpi); scores are scaled by qscale (1/sqrt(128)); softmax in fp32.
 *   out fp16 [B, Hq, 128]; lse optional float [B, Hq] (log-sum-exp of the scaled scores).
 */
size_t gear_attn_decode_workspace(int B, int Hq, int T, int bits);
int gear_attn_decode(const void* q, const void* kcode, const void* kscale, const void* kmn, const void* kP, const void* kQ,
                     const void* koidx, const void* koval, const void* vcode, const void* vscale, const void* vmn,
                     const void* vP, const void* vQ, const void* voidx, const void* voval, const void* kwin,
                     const void* vwin, int B, int Hq, int Hkv, int D, int T, int W, int ldk, int lsk, int tcap_v, int tf_k,
                     int tf_v, int group, int bits, int mode, int rk, int rv, int kk, int kv, float qscale, void* out,
                     void* lse, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the uncompressed baseline: single-token attention over an fp16 cache --------------------------------------
 * What the reference's harness runs as model "None" beside gearl / KIVI (cuda_supported_gear/test.py:41-62: HF attention
 * over the fp16 past_key_values) -- same flash-decoding split, same merge kernel and same grouped-query mapping as
 * gear_attn_decode, so that bench.py can put a compressed and an uncompressed time per token side by side.
 *   q fp16 [B, Hq, 128]; k, v fp16 [B, Hkv, tcap, 128], tokens [0, T) valid, 0 < T <= min(tcap, 8320); qscale = 1/sqrt(128)
 *   out fp16 [B, Hq, 128]; lse optional float [B, Hq]; workspace: gear_attn_decode_workspace(B, Hq, T, any bits).
 */
int gear_attn_decode_f16(const void* q, const void* k, const void* v, int B, int Hq, int Hkv, int D, int T, int tcap,
                         float qscale, void* out, void* lse, void* workspace, size_t workspace_bytes, void* stream);

/* ---- decode attention with per-segment low-rank factors (the streaming cache of the attention hook) ----------
 * As gear_attn_decode, but the channel-side factors kP / vP are [nseg, B*Hkv, 128, r]: tokens [0, seg0) use set 0 (the
 * prefill block, cuda_supported_gear/modeling_llamagear.py:402-434), every following `seglen` tokens their own set (the
 * 64-token decode blocks stacked on a leading buffer dim in the reference, :276-286).  seglen == 0: one segment.
 * wcap: row pitch (tokens) of kwin / vwin, >= W (a pre-allocated window buffer).
 */
int gear_attn_decode_seg(const void* q, const void* kcode, const void* kscale, const void* kmn, const void* kP,
                         const void* kQ, const void* koidx, const void* koval, const void* vcode, const void* vscale,
                         const void* vmn, const void* vP, const void* vQ, const void* voidx, const void* voval,
                         const void* kwin, const void* vwin, int B, int Hq, int Hkv, int D, int T, int W, int ldk, int lsk,
                         int tcap_v, int tf_k, int tf_v, int group, int bits, int mode, int rk, int rv, int kk, int kv,
                         int seg0, int seglen, int wcap, float qscale, void* out, void* lse, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- per-token glue of a decode step (one launch each) ---------------------------------------------------------
 * gear_rope_append: qkv fp16 [B, (Hq + 2 Hkv) * 128] (fused q/k/v projection of the new token) -> RoPE at `pos` on q and k
 *   (modeling_llamagear.py:203-205), q_out fp16 [B, Hq, 128], k / v written to slot `slot` of the fp16 residual window
 *   kwin / vwin [B*Hkv, W, 128] (the torch.cat of :256, :316).
 * gear_add_rmsnorm: res_out = res_in + delta (delta may be NULL), y = weight * rmsnorm(res_out)   (LlamaRMSNorm + residual)
 * gear_silu_mul: out = silu(gate) * up for gate_up = [B, 2 I]                                         (LlamaMLP)
 */
int gear_rope_append(const void* qkv, int B, int Hq, int Hkv, int D, int pos, float theta, void* q_out, void* kwin,
                     void* vwin, int slot, int W, void* stream);
int gear_add_rmsnorm(const void* res_in, const void* delta, const void* weight, int64_t rows, int H, float eps,
                     void* res_out, void* y, void* stream);
int gear_silu_mul(const void* gate_up, int64_t B, int I, void* out, void* stream);

/* ---- device-side decode state (hipGraph-replayable token step) ---------------------------------------------------
 * state = int32[4] {pos, slot, T, W} in device memory: position of the token being processed, its slot in the fp16 window,
 * number of compressed tokens, number of window tokens INCLUDING that token (W = slot + 1).  The _dyn entry points read the per-token scalars from
 * it so that a captured graph of the whole token step can be replayed unchanged; gear_decode_state_advance() moves it on
 * by one token (pos, slot, W += 1).  gear_attn_decode_dyn plans its grid for `T` = the cache capacity; chunks beyond the
 * current length exit at once.  With dyn_state == NULL they behave exactly like the static entry points.
 */
int gear_attn_decode_dyn(const void* q, const void* kcode, const void* kscale, const void* kmn, const void* kP,
                         const void* kQ, const void* koidx, const void* koval, const void* vcode, const void* vscale,
                         const void* vmn, const void* vP, const void* vQ, const void* voidx, const void* voval,
                         const void* kwin, const void* vwin, int B, int Hq, int Hkv, int D, int T, int W, int ldk, int lsk,
                         int tcap_v, int tf_k, int tf_v, int group, int bits, int mode, int rk, int rv, int kk, int kv,
                         int seg0, int seglen, int wcap, const void* dyn_state, float qscale, void* out, void* lse,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Chunk index of sorted outlier lists (the build's own addition to the sparse payload; the reference's fused path stores no
 * outliers at all, modeling_llamagear.py cache slots 11-12 / 15-16 are None).  oidx: uint16 [n_lists][k], every list
 * ascending; out: uint8 [n_lists][n_bounds], out[l][b] = first position of list l whose index is >= b * step.
 *   K payload: lists = (b, h, d, side), step 128 (tokens), n_bounds = ceil(T / 128) + 1
 *   V payload: lists = (b, t, side),    step 128 (columns = one KV head), n_bounds = Hkv + 1
 * gear_attn_decode_idx = gear_attn_decode with the two index tables (either may be NULL): a 128-token chunk then finds its
 * outliers with two byte loads per list instead of a binary search (contexts <= 8192 tokens; ignored otherwise). */
int gear_outlier_chunk_index(const void* oidx, int64_t n_lists, int k, int step, int n_bounds, void* out, void* stream);
int gear_attn_decode_idx(const void* q, const void* kcode, const void* kscale, const void* kmn, const void* kP, const void* kQ,
                         const void* koidx, const void* koval, const void* kochunk, const void* vcode, const void* vscale,
                         const void* vmn, const void* vP, const void* vQ, const void* voidx, const void* voval,
                         const void* vochunk, const void* kwin, const void* vwin, int B, int Hq, int Hkv, int D, int T, int W,
                         int ldk, int lsk, int tcap_v, int tf_k, int tf_v, int group, int bits, int mode, int rk, int rv,
                         int kk, int kv, float qscale, void* out, void* lse, void* workspace, size_t workspace_bytes,
                         void* stream);
/* ---- the streaming cache as one view --------------------------------------------------------------------------------
 * A pre-allocated cache of one layer (or of several layers riding in the batch dimension) that blocks are appended to in place
 * by gear_compress_key_fused / gear_compress_value_fused.  tcap = token capacity of every per-token tensor.
 *   K outlier lists koidx / koval [B*Hkv, 128, 2, kk_cap]: of every (channel, side) list the first kk0 + kkb * ((T - seg0) / seglen)
 *   entries are valid (kk0 from the prompt segment, kkb appended per block; later blocks hold later tokens, so the lists stay
 *   sorted); V lists voidx / voval [B, tcap, 2 kv].  Optional accelerators, all derived from the lists:
 *   kochunk uint8 [B*Hkv*128*2][nbk_pitch] / vochunk uint8 [B*tcap*2][Hkv+1]   chunk indices (gear_outlier_chunk_index_ex)
 *   ktile uint32 [B*Hkv][nck][ktile_cap] + kcnt int32 [B*Hkv][nck], vtile uint32 [B*Hkv][nblk][vtile_cap] + vcnt   sparse tiles
 *   (gear_cache_tiles_build): the outlier corrections value - dequant of a 128-token chunk / 64-token block as a flat list.
 */
typedef struct gear_cache_view {
    const void *kcode, *kscale, *kmn, *kP, *kQ, *koidx, *koval;
    const void *vcode, *vscale, *vmn, *vP, *vQ, *voidx, *voval;
    const void *kwin, *vwin;
    const void *kochunk, *vochunk;
    void *ktile, *kcnt, *vtile, *vcnt;
    int B, Hkv, D, tcap, ldk, lsk, group, bits, mode, rk, rv;
    int kk_cap, kk0, kkb, kv, seg0, seglen, wcap, nbk_pitch;
    int ktile_cap, nck, vtile_cap, nblk;
} gear_cache_view;

/* Single-token decode attention over a cache view: gear_attn_decode_dyn's arithmetic (segment factors, fp16 window of W <= 128
 * tokens with row pitch wcap, optional device-side {pos, slot, T, W}), outliers through the tiles when present (no search, no
 * dependent loads), else through the chunk indices, else by binary search in the lists. */
int gear_attn_decode_cache(const gear_cache_view* c, const void* q, int Hq, int T, int W, const void* dyn_state, float qscale,
                           void* out, void* lse, void* workspace, size_t workspace_bytes, void* stream);
/* ---- chunk attention: extend a cache by n tokens at once -----------------------------------------------------------------
 * Replaces n single-token decode steps (n x gear_attn_decode_cache, each reading the whole compressed prefix) when a block of
 * tokens enters a cache that already holds T compressed + W window tokens (second chat turn, speculative verification, a prompt
 * that arrives in parts).  Query i (0 <= i < n) attends with one fp32 softmax over the T compressed tokens (reconstructed as
 * gear_attn_decode_cache does: dequant, stored outlier values in place of the dequantized ones, + Q P^T of the token's factor
 * segment), the W window tokens and the chunk's own rows 0 .. i (causal).  Changes no cache state.
 *   c      the cache view (mode 0, bits 2 / 4, group 32 / 64, rank <= 16, T % 64 == 0, W <= wcap; outliers from the lists)
 *   q      fp16 [B, Hq, n, 128]; k_new / v_new fp16 [B, Hkv, n, 128] (post-RoPE), 1 <= n <= 2048, Hq % Hkv == 0
 *   out    fp16 [B, Hq, n, 128]; lse optional float [B, Hq, n] (log-sum-exp of the scaled scores)
 *   workspace: gear_attn_extend_workspace(B, Hq, n, T, W) bytes (bounds every Hkv that divides Hq).  Two launches. */
size_t gear_attn_extend_workspace(int B, int Hq, int n, int T, int W);
int gear_attn_extend_cache(const gear_cache_view* c, const void* q, int Hq, int n, int T, int W, const void* k_new,
                           const void* v_new, float qscale, void* out, void* lse, void* workspace, size_t workspace_bytes,
                           void* stream);
/* ---- speculative verify: n <= 16 draft tokens at once -----------------------------------------------------------------------
 * gear_attn_extend_cache's semantics (query i over the T compressed tokens, the W window tokens and chunk rows 0 .. i, one fp32
 * softmax, no cache state changes) for the draft sizes of speculative decoding, on the decode kernels: q goes to the decode
 * partial dispatch as B x (Hq n) query rows of one token each (a KV head's G n rows share its compressed chunks), and one merge
 * launch adds the window and the causal chunk rows.  Accepts every configuration gear_attn_decode_cache accepts (T == 0 and W == 0
 * included); W + n may exceed wcap (the chunk rows are never written into the window).  The attention options apply as for decode,
 * except attn_fold (the merge always runs in its own launch).
 *   q      fp16 [B, Hq, n, 128] at positions T + W .. T + W + n - 1; k_new / v_new fp16 [B, Hkv, n, 128] (post-RoPE), 1 <= n <= 16
 *   out    fp16 [B, Hq, n, 128]; lse optional float [B, Hq, n] (log-sum-exp of the scaled scores)
 *   workspace: gear_attn_verify_workspace(B, Hq, n, T, W) bytes.  Two launches (one when T == 0). */
size_t gear_attn_verify_workspace(int B, int Hq, int n, int T, int W);
int gear_attn_verify_cache(const gear_cache_view* c, const void* q, int Hq, int n, int T, int W, const void* k_new,
                           const void* v_new, float qscale, void* out, void* lse, void* workspace, size_t workspace_bytes,
                           void* stream);
/* ---- tree verify: the n <= 16 rows are the nodes of a draft tree -------------------------------------------------------------
 * gear_attn_verify_cache with one change: output row (b, hq, i) is one fp32 softmax over the T compressed tokens, the W window
 * tokens and those chunk rows j whose bit j is set in anc[b, i] (row i's ancestors in the tree and row i itself), not chunk rows
 * 0 .. i.  The caller lists the nodes in a topological order (bit j set only for j <= i, bit i set); the kernel does not rely on
 * it and uses m = (anc[b, i] | 1u << i) & ((2u << i) - 1): no mask gives an empty softmax or lets a row read a row after itself.
 * A masked row is skipped, not weighted by zero; the rows that remain are added in gear_attn_verify_cache's order, so the chain
 * mask (2u << i) - 1 repeats its arithmetic.  The compressed part runs through the same partial dispatch (the mask does not touch
 * it); arguments, checks, options and launches are gear_attn_verify_cache's, plus
 *   anc    uint32 [B, n], device (not NULL)
 *   workspace: gear_attn_verify_tree_workspace(B, Hq, n, T, W) bytes (= gear_attn_verify_workspace). */
size_t gear_attn_verify_tree_workspace(int B, int Hq, int n, int T, int W);
int gear_attn_verify_tree(const gear_cache_view* c, const void* q, int Hq, int n, int T, int W, const void* k_new,
                          const void* v_new, const void* anc, float qscale, void* out, void* lse, void* workspace,
                          size_t workspace_bytes, void* stream);
/* ---- shared-prefix decode: S sequences over ONE stored prompt ----------------------------------------------------------------
 * `prefix` is a view with B == 1 that holds the prompt's Tp compressed tokens (no window is read from it); `tail` is a view with
 * B == S of the same configuration (Hkv, D, bits, group, mode, ranks) that holds what every sequence appended since: T compressed
 * tokens and W window tokens each (all sequences advance in lockstep).  Output row (s, hq) is ONE fp32 softmax over the prefix's Tp
 * tokens, then sequence s's T compressed tokens, then its W window rows.  The S Hq query rows go over the prefix through the decode
 * partial dispatch as rows of its KV heads -- (Hq / Hkv) S rows share a KV head's chunks as a grouped-query group would; a
 * workgroup serves 8 / 4 / 2 / 1 consecutive rows of them, q is addressed in place --, the tails go through the ordinary dispatch
 * (skipped when T == 0), and one merge launch joins both sets of partial results with the window rows.  The attention options
 * apply as for decode, except attn_fold.  No cache state changes.  The same call on the same data gives the same bits every time
 * (sampled decoding with one seed repeats): the vector kernels run here with their outlier sums as integer sums.
 *   Tp     positive multiple of 64, <= prefix->tcap;  T multiple of 64 in [0, tail->tcap];  0 <= W <= tail->wcap <= 128
 *   q      fp16 [S, Hq, 128], Hq % Hkv == 0, S Hq <= 65535;  out fp16 [S, Hq, 128];  lse optional float [S, Hq]
 *   workspace: gear_attn_decode_shared_workspace(S, Hq, Tp, T, bits) bytes.  Three launches (two when T == 0). */
size_t gear_attn_decode_shared_workspace(int S, int Hq, int Tp, int T, int bits);
int gear_attn_decode_shared(const gear_cache_view* prefix, int Tp, const gear_cache_view* tail, int T, int W, const void* q, int Hq,
                            float qscale, void* out, void* lse, void* workspace, size_t workspace_bytes, void* stream);
/* ---- shared-prefix extend: n tokens per sequence behind ONE stored prompt (system-prompt serving) -----------------------------
 * gear_attn_extend_cache for S sequences that share a prompt: `prefix` (B == 1, Tp compressed tokens, its window is not read) and
 * `tail` (B == S, same Hkv, D, bits, group, mode, ranks; T compressed + W window tokens per sequence, all in lockstep) as for
 * gear_attn_decode_shared.  Output row (s, hq, i) is ONE fp32 softmax over the prefix's Tp tokens, then sequence s's T compressed
 * tokens, then its W window rows, then its own chunk rows 0 .. i -- every term reconstructed as gear_attn_extend_cache does.  Three
 * launches: the chunk kernel over the prefix with the batch folded into the row axis (S n Hq / Hkv rows per KV head, row
 * (s n + i) (Hq / Hkv) + gh, q addressed in place, no mask: a 64-token prefix piece is read and dequantized once per 64 query rows
 * of ANY sequences), the chunk kernel over the tail view (tail-local causality), and one merge of both sets of partial results.
 * No cache state changes; no float atomics: the same call on the same data gives the same bits every time.
 *   Tp     positive multiple of 64, <= prefix->tcap;  T multiple of 64 in [0, tail->tcap];  0 <= W <= tail->wcap
 *   q      fp16 [S, Hq, n, 128]; k_new / v_new fp16 [S, Hkv, n, 128] (post-RoPE), 1 <= n <= 2048, Hq % Hkv == 0, S Hkv <= 65535,
 *          Tp + T + W + n <= 65535
 *   out    fp16 [S, Hq, n, 128]; lse optional float [S, Hq, n] (log-sum-exp of the scaled scores)
 *   workspace: gear_attn_extend_shared_workspace(S, Hq, n, Tp, T, W) bytes: both passes' partial slots (bounds every Hkv that
 *          divides Hq; 0 for an invalid shape). */
size_t gear_attn_extend_shared_workspace(int S, int Hq, int n, int Tp, int T, int W);
int gear_attn_extend_shared(const gear_cache_view* prefix, int Tp, const gear_cache_view* tail, int T, int W, const void* q, int Hq,
                            int n, const void* k_new, const void* v_new, float qscale, void* out, void* lse, void* workspace,
                            size_t workspace_bytes, void* stream);
/* ---- beam search: gather the per-sequence state of a cache along its batch axis, in place ---------------------------------------
 * After the call the live state of sequence b in every layer is what the live state of sequence src_idx[b] was before it, bit for
 * bit, for every field the view has (the reference reorders its tuple cache through Hugging Face's _reorder_cache, one
 * index_select per tensor; this cache is pre-allocated and pooled, so the gather runs in place over the live ranges only).
 *   c        the pooled view with B = n_layers * batch (fields [n_layers, batch, ...]; kP / vP [n_layers, nseg, batch, ...]), or one
 *            cache's view with n_layers = 1; the tensors behind the const pointers are WRITTEN
 *   T, W     compressed tokens (multiple of 64, <= tcap) and window tokens (<= wcap) of every sequence: what is copied is codes /
 *            scale / mn / token factors / V lists of the first T tokens, the first kk0 + kkb (T - seg0) / seglen entries of every K
 *            list, the factor segments written so far, the tiles of the chunks / blocks that hold tokens, the first W window rows
 *   src_idx  DEVICE int32 [batch], read on the device (no host synchronisation); repeats and cycles are allowed; a sequence with
 *            src_idx[b] == b is not touched; an entry outside [0, batch) is treated as b
 *   workspace: gear_cache_reorder_workspace(c, n_layers, batch, T, W) bytes (the live ranges of all sequences; 0 for an invalid
 *            shape).  Two launches: sources -> workspace, workspace -> destinations (a destination may be another row's source). */
size_t gear_cache_reorder_workspace(const gear_cache_view* c, int n_layers, int batch, int T, int W);
int gear_cache_reorder(const gear_cache_view* c, int n_layers, int batch, int T, int W, const int32_t* src_idx, void* workspace,
                       size_t workspace_bytes, void* stream);
/* ---- snapshots: the live per-sequence state of a cache as one packed blob, and back ----------------------------------------------
 * The blob is the live state (the fields and live ranges gear_cache_reorder moves, same c / n_layers / batch / T / W) of sequences
 * seq0 .. seq0 + n_seq - 1 of every layer.  It has no header -- the caller keeps T, W, seg0 and kk0.  Layout: the fields in the
 * order kcode, kscale, kmn, vcode, vscale, vmn, kP, kQ, vP, vQ, koidx, koval, kochunk, voidx, voval, vochunk, ktile, kcnt, vtile,
 * vcnt, kwin, vwin (those the view has); within a field (outer index = layer [, factor segment], sequence, row); each row its live
 * bytes rounded up to 16 (the padding is zero); rows that are live to their end, or whose pitch lies within one 128-byte line, are
 * one run per sequence.  The layout is a function of (the view's geometry, kk0, seg0, n_layers, T, W, n_seq) alone.
 *   gear_cache_snapshot_bytes: the blob's size (a multiple of 16, linear in n_seq; host only; 0 for an invalid shape)
 *   gear_cache_snapshot: fields -> blob, ONE launch
 *   gear_cache_restore:  blob -> fields of sequences seq0 .. seq0 + n_seq - 1, ONE launch.  blob_seqs == n_seq: sequence j of the
 *            blob goes to sequence seq0 + j; blob_seqs == 1: the blob's one sequence goes to all n_seq destinations (a fork);
 *            anything else is an argument error.  Only the live ranges of the destination sequences are written.
 *   blob     DEVICE memory, 16-byte aligned (anything else is an argument error), at least gear_cache_snapshot_bytes(c, n_layers,
 *            batch, T, W, n_seq resp. blob_seqs) bytes
 * Neither call reads an index from device memory or synchronises. */
size_t gear_cache_snapshot_bytes(const gear_cache_view* c, int n_layers, int batch, int T, int W, int n_seq);
int gear_cache_snapshot(const gear_cache_view* c, int n_layers, int batch, int T, int W, int seq0, int n_seq, void* blob,
                        size_t blob_bytes, void* stream);
int gear_cache_restore(const gear_cache_view* c, int n_layers, int batch, int T, int W, int seq0, int n_seq, const void* blob,
                       size_t blob_bytes, int blob_seqs, void* stream);
/* (Re)build the sparse tiles of K chunks [k_chunk0, k_chunk1) (128 tokens each) and V blocks [v_blk0, v_blk1) (64 tokens each) of a
 * cache that holds T compressed tokens: called after the prompt and after every appended block (the chunk the block lies in). */
int gear_cache_tiles_build(const gear_cache_view* c, int T, int k_chunk0, int k_chunk1, int v_blk0, int v_blk1, void* stream);
/* ---- the decode-time block boundary in ONE launch -------------------------------------------------------------------------
 * Replaces, for the 64-token block the attention hook compresses whenever its fp16 window is full
 * (cuda_supported_gear/modeling_llamagear.py:265-286 key_compression of the block, :335-378 value_compression; with a sparsity
 * in the config also gears_channelQ / gears_tokenQ of GenerationBench/.../Simulated/compress_function.py:261-333 on the block),
 * the sequence gear_compress_key_fused + gear_compress_value_fused + gear_outlier_chunk_index_ex + gear_cache_tiles_build (~10
 * launches): one wave per (layer*batch, head, K | V) tile of 64 x 128 fp16 reads the window (c->kwin / c->vwin, row pitch wcap),
 * selects the outliers (K: kkb per side and channel over the 64 tokens; V: kv per side and token row ACROSS the heads, found by
 * "row duty" waves of the same launch and handed to the V tiles through sync_ws), quantizes (fp16-stepwise arithmetic, mode 0),
 * packs, keeps the error tile in LDS and runs the rank-r power iteration on it (token side: G' = E E^T is 64 x 64), then writes
 * codes / scale / mn / lists / chunk-index bytes / sparse tiles / factors at token offset t_off of the view's tensors in place.
 *   c       the cache view with B = layers * batch; mode must be 0, D 128, Hkv <= 64, kkb <= 16; the tensors behind the const
 *           pointers are WRITTEN (token rows t_off .. t_off + 63, K list positions o_off .. o_off + kkb - 1, tile of the chunk /
 *           block the tokens lie in)
 *   P0k / P0v float [B*Hkv, 128, rk | rv] initial bases; kP_out / vP_out fp16, head bh at element offset
 *           (bh / p_inner) * outer_stride + (bh % p_inner) * 128 * r (the per-segment factor tensors of the cache)
 *   sync_ws gear_compress_block_workspace(B, Hkv) bytes of device memory, ZEROED ONCE by the caller and then left alone (row
 *           flags carry a per-call tag); the word at gear_compress_block_status_ptr(sync_ws) becomes non-zero if a V tile ever
 *           gave up waiting for its rows (never on a healthy device; the call then does not hang, its V outliers are wrong).
 * Payload (codes, scale, mn, outlier sets and values, chunk index, tile contents) is bit-identical to the chain's; the factors
 * span the same subspaces (Q P^T within fp16 rounding of the chain's). */
size_t gear_compress_block_workspace(int64_t B, int Hkv);
int gear_compress_block(const gear_cache_view* c, int t_off, int o_off, int loop, const void* P0k, const void* P0v, void* kP_out,
                        void* vP_out, int64_t p_inner, int64_t kp_outer_stride, int64_t vp_outer_stride, void* sync_ws,
                        size_t sync_ws_bytes, void* stream);
const void* gear_compress_block_status_ptr(const void* sync_ws);

/* gear_compress_key_fused's single-read kernel (csrc/kone.hip; fp32 arithmetic, prompt-size tensors) exchanges outlier candidates
 * between the workgroups of a head inside ONE launch; every wait of that exchange is bounded.  Returns how many waits ran into their
 * bound since the library was loaded -- 0 on a healthy device; anything else means the payload of that call is invalid (the device
 * could not co-schedule a head's workgroups).  Replaces nothing in the reference (it has no in-kernel exchange).  Synchronises the
 * device.  -1: the query itself failed. */
int gear_kone_timeouts(void);
/* Heads of single-read-kernel calls whose outlier threshold guess failed and which the exact kernel chain redid (cumulative since the
 * library was loaded; 0 on ordinary data; results are exact either way).  Synchronises the device.  -1: the query failed. */
int gear_kone_fallback_heads(void);
/* Chunk index over lists that live inside larger tensors (the streaming cache keeps its tables up to date block by block):
 * lists (o, i), o < n_outer, i < inner, list id = o * outer_pitch + first + i; list `id` is oidx + id * list_stride with k valid
 * entries; out[id * out_pitch + b] = first position whose index is >= b * step, b < n_bounds.
 *   kochunk of a gear_cache_view: the prompt segment's entries of the K lists (k = kk0, list_stride = kk_cap, pitch nbk_pitch)
 *   vochunk: one row of H + 1 bounds per (token row, side) of the V lists. */
int gear_outlier_chunk_index_ex(const void* oidx, int64_t n_outer, int64_t inner, int64_t outer_pitch, int64_t first, int k,
                                int list_stride, int step, int n_bounds, void* out, int out_pitch, void* stream);
int gear_rope_append_dyn(const void* qkv, int B, int Hq, int Hkv, int D, const void* dyn_state, float theta, void* q_out,
                         void* kwin, void* vwin, int W, void* stream);
int gear_decode_state_advance(void* state, void* stream);

/* ---- fp16 GEMV for the decode token step: y[b, n] = sum_k x[b, k] W[n, k], 1 <= B <= 4, K % 8 == 0 -------------------
 * (torch.nn.functional.linear for one token; used by FastGearDecoder for the q/k/v, o, gate/up, down and lm_head GEMVs)
 */
int gear_gemv_f16(const void* x, const void* W, int B, int K, int N, void* y, void* stream);
/* y = res_in + W x (the residual-stream update after o_proj / down_proj); y may alias res_in, not x */
int gear_gemv_f16_add(const void* x, const void* W, int B, int K, int N, const void* res_in, void* y, void* stream);

/* Fused token-step projections (same 1 <= B <= 4, K % 8 == 0).  They fold the glue launches of a decoder layer
 * (cuda_supported_gear/modeling_llamagear.py:502-560: input_layernorm / post_attention_layernorm, :193-205 q/k/v + rotary,
 * LlamaMLP act_fn(gate) * up) into the weight stream:
 *   gear_gemv_f16_norm : v = x + delta (delta may be NULL; otherwise res_out [B,K] receives v and must not alias x/delta);
 *                        y = W . (norm_w * v) * rsqrt(mean(v^2) + eps)  (norm_w NULL: already folded into W's columns).   swiglu = 1: W rows are interleaved
 *                        (gate_0, up_0, gate_1, up_1, ...), swiglu = 2: blocked [N/2 gate rows | N/2 up rows] (gate_proj / up_proj
 *                        as the modules hold them); y [B, N/2] = fp16(silu(gate)) * up.
 *   gear_gemv_qkv_rope : the same prologue, W = [q heads | k heads | v heads] x 128 rows; RoPE (HF rotate_half, fp16 op by
 *                        op) on q and k at `pos`; q -> q_out [B,Hq,128]; k, v -> window slot `slot` of kwin / vwin
 *                        [B*Hkv, wcap, 128].  dyn_state != NULL: pos and slot are read from the device state
 *                        {pos, slot, T, W} (hipGraph replay).
 */
int gear_gemv_f16_norm(const void* x, const void* delta, const void* norm_w, float eps, const void* W, int B, int K, int N,
                       int swiglu, void* res_out, void* y, void* stream);
int gear_gemv_qkv_rope(const void* x, const void* delta, const void* norm_w, float eps, const void* Wqkv, int B, int K,
                       int Hq, int Hkv, int D, int pos, int slot, int wcap, float theta, const void* dyn_state,
                       void* res_out, void* q_out, void* kwin, void* vwin, void* stream);

/* ---- token sampling: temperature, top-k, top-p and speculative accept / residual in ONE launch ------------------------------
 * The decoders' replacement for the argmax (HF's generate(do_sample=True, temperature, top_k, top_p), the settings the reference
 * evaluates with: GenerationBench/GenerationTest/evaluation_bbh_cot.py:381-390).  One workgroup per row; never synchronises or
 * allocates (graph-capturable).
 *   logits  fp16 [rows, V] (fp32 when logits_fp32), row stride ld >= V elements; 1 <= V <= 262144
 *   row r   belongs to sequence b = r / n_per_seq at position P = pos + r % n_per_seq, pos = *pos_dev + pos0 (pos_dev: device int32,
 *           e.g. the decode state {pos, ...}) or pos0 when pos_dev is NULL
 *   params  (host pointer) temperature >= 0, top_k >= 0 (0 or >= V: off), top_p in (0, 1] (1: off), seed
 *   draft   optional int64 [rows]: the drafted token of the row, -1 = none;  u optional float [rows][2]: (draw, accept) uniforms
 *           in place of the generator
 *   token_out int64 [rows]; accepted_out optional int32 [rows] (1: the draft was accepted); logprob_out optional float [rows]
 *           (log p of the emitted token under the filtered distribution; 0 for temperature 0)
 * Semantics (HF warper order): temperature 0 = argmax (first index), a draft accepted iff it equals it.  Otherwise
 * x = fp32(logit) / temperature, -inf never kept; top-k keeps x >= the k-th largest x (edge ties kept); top-p keeps x_i iff the
 * softmax mass (over the kept set) of the values > x_i is < top_p; e_j = exp(x_j - max), Z = sum over the kept set; the draw is the
 * smallest kept index whose running sum in index order exceeds u_draw Z.  Draft rows: accept iff u_acc < e_d / Z; a rejected row
 * draws over the kept set without d.  Uniforms: Philox4x32-10, key (seed lo, seed hi), counter (P, b, 0 = draw / 1 = accept, 0),
 * u = (out[0] >> 8) 2^-24 -- a pure function of (seed, sequence, position, logits).  Integer sums only: bit-reproducible. */
typedef struct {
    float temperature;
    int top_k;
    float top_p;
    int reserved;
    uint64_t seed;
} gear_sample_params;
int gear_sample_tokens(const void* logits, int logits_fp32, int rows, int V, int64_t ld, int n_per_seq,
                       const gear_sample_params* p, const int* pos_dev, int pos0, const int64_t* draft, const float* u,
                       int64_t* token_out, int32_t* accepted_out, float* logprob_out, void* stream);

/* ---- the exchange step of the head-sharded decode path (the reference has no distributed code) -------
 * With the KV heads split across ranks (one process per GPU) the only data any rank needs from the others is their slice of
 * the attention output in front of o_proj (cuda_supported_gear/modeling_llamagear.py:478-482 merges the heads).  Instead of a
 * collective call per layer per token, every rank owns an "exchange area" of uncached device memory that its peers map with
 * hipIpc (xGMI peer memory; the same calls work between two processes on one GPU, which is how the tests run it) and
 * gear_xchg_allgather is ONE single-workgroup launch that stores the local slice into every area, raises a flag, waits for
 * the peers' flags and copies the gathered rows out -- nothing in it needs the host, so it lives inside the hipGraph of the
 * token step.
 *   gear_xchg_bytes     size of an area for `world` ranks and slices of bytes_per_rank (0: world out of range, max 64)
 *   gear_xchg_alloc     uncached, zeroed, exportable; gear_xchg_free releases it (after the peers closed their mappings)
 *   gear_xchg_export    64-byte handle to send to the peers (any byte transport); gear_xchg_open maps a peer's area in this
 *                       process, gear_xchg_close unmaps it
 *   gear_xchg_allgather src [rows, row_bytes] of this rank -> out [rows, world, row_bytes] (rank r's bytes at slot r of every
 *                       row); peers = DEVICE array of `world` area pointers as mapped in this process (peers[rank] = the own
 *                       area); row_bytes % 16 == 0.  Every rank must issue the same sequence of calls.  A rank whose peers do
 *                       not show up within 3 s sets bit 0 of *status (device int32, may be NULL) and returns garbage rather
 *                       than hang. */
size_t gear_xchg_bytes(int world, size_t bytes_per_rank);
int gear_xchg_alloc(size_t bytes, void** ptr);
int gear_xchg_free(void* ptr);
int gear_xchg_export(const void* ptr, void* handle64);
int gear_xchg_open(const void* handle64, void** ptr);
int gear_xchg_close(void* ptr);
int gear_xchg_allgather(const void* src, int rows, size_t row_bytes, int world, int rank, const void* peers, void* out,
                        void* status, void* stream);

/* ---- the KIVI cache on the fused decode path (csrc/kivi.hip) ---------------------------------------------------------------------
 * The KIVI baseline's state machine (K: an fp16 window quantized per channel as one block of R tokens; V: a sliding fp16 window whose
 * oldest token is quantized per token) on a pre-allocated cache.  A gear_cache_view describes it: kcode / kscale / kmn and vcode /
 * vscale / vmn with the layouts of the streaming cache (no factors, no outlier lists: rk = rv = kv = kk_cap = 0), wcap = R, kwin =
 * the K window fp16 [B*Hkv, R, 128] (token t >= Tk in row t - Tk) and vwin = the V RING fp16 [B*Hkv, R + 1, 128]: token t lives in
 * row t % (R + 1), so the row token n overwrites holds token n - (R + 1).  bits 2 / 4, group 64, R 64 / 128, mode 0.
 *
 * gear_kivi_rope_append: gear_rope_append for this cache -- qkv fp16 [B, (Hq + 2 Hkv) * 128] -> RoPE at `pos` on q and k, q to
 *   q_out [B, Hq, 128], k into row kslot of the K window, v into ring row n % (R + 1) (n = the token's index in the sequence).
 *   evict_row = n - (R + 1): in the same launch, before the overwrite, the ring row's old contents (token n - (R + 1)) are
 *   quantized per token (groups of 64 channels, fp16 scale and minimum, gear_quant_pack_lastdim's fp16-stepwise arithmetic) into
 *   row evict_row of vcode / vscale / vmn [B*Hkv, tcap, ...]; evict_row = -1: nothing is evicted (the ring is not full yet, or
 *   the prompt's prefill packed that row already).  One launch.
 * gear_kivi_append: the same for rows that are already rotated, k_new / v_new fp16 [B, Hkv, 128].
 * gear_attn_decode_kivi: q fp16 [B, Hq, 128] -> out fp16 [B, Hq, 128] (lse optional float [B, Hq]): ONE fp32 softmax over the L
 *   tokens -- K from the codes for [0, Tk) and from the window for [Tk, L), V from the codes for [0, Nv) and from the ring for
 *   [Nv, L).  Tk % R == 0, 0 <= L - Tk <= R, 0 <= L - Nv <= R + 1, Nv rounded down to 64 must not exceed Tk.  The whole 64-token
 *   chunks below Nv go through the decode partial dispatch, one seam kernel per output row scores the remaining <= 63 + R + 1
 *   tokens and merges: two launches (one when Nv < 64), whatever L is.  No cache state changes; the same call on the same data
 *   gives the same bits.  workspace: gear_attn_decode_kivi_workspace(B, Hq, T, bits) bytes for any T >= Nv (0: bad arguments). */
int gear_kivi_rope_append(const void* qkv, int B, int Hq, int Hkv, int D, int pos, float theta, void* q_out, void* kwin, int kslot,
                          void* vring, int n, int R, int evict_row, void* vcode, void* vscale, void* vmn, int tcap, int group,
                          int bits, void* stream);
int gear_kivi_append(const void* k_new, const void* v_new, int B, int Hkv, int D, void* kwin, int kslot, void* vring, int n, int R,
                     int evict_row, void* vcode, void* vscale, void* vmn, int tcap, int group, int bits, void* stream);
size_t gear_attn_decode_kivi_workspace(int B, int Hq, int T, int bits);
int gear_attn_decode_kivi(const gear_cache_view* c, const void* q, int Hq, int L, int Tk, int Nv, float qscale, void* out, void* lse,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- RoPE scaling (config.rope_scaling: linear / llama3 / yarn): the frequency-table flavours of the RoPE entry points -------
 * Each takes its parent's arguments with `float theta` replaced by `const float* inv_freq` -- a DEVICE pointer to the 64 fp32
 * inverse frequencies of the rotation pairs (gear_amd/rope.py: rope_parameters) -- and `float attn_factor` (yarn's cos / sin
 * scale; 1 otherwise):  ang = (float)pos * inv_freq[p], cos = fp16(cosf(ang) * attn_factor), sin alike, then the parent's fp16
 * op-by-op rotation.  Everything else -- V copy, window / ring writes, the KIVI eviction, the device state of the dyn flavours --
 * is the parent's code (one kernel template, `bool TAB`).  A null table and an attn_factor that is not positive and finite are
 * refused before any launch, as is whatever the parent refuses.  The table is read at run time: a captured graph keeps the
 * pointer, so the buffer must outlive it. */
int gear_rope_append_freq(const void* qkv, int B, int Hq, int Hkv, int D, int pos, const float* inv_freq, float attn_factor,
                          void* q_out, void* kwin, void* vwin, int slot, int W, void* stream);
int gear_rope_append_dyn_freq(const void* qkv, int B, int Hq, int Hkv, int D, const void* dyn_state, const float* inv_freq,
                              float attn_factor, void* q_out, void* kwin, void* vwin, int W, void* stream);
int gear_gemv_qkv_rope_freq(const void* x, const void* delta, const void* norm_w, float eps, const void* Wqkv, int B, int K,
                            int Hq, int Hkv, int D, int pos, int slot, int wcap, const float* inv_freq, float attn_factor,
                            const void* dyn_state, void* res_out, void* q_out, void* kwin, void* vwin, void* stream);
int gear_kivi_rope_append_freq(const void* qkv, int B, int Hq, int Hkv, int D, int pos, const float* inv_freq, float attn_factor,
                               void* q_out, void* kwin, int kslot, void* vring, int n, int R, int evict_row, void* vcode,
                               void* vscale, void* vmn, int tcap, int group, int bits, void* stream);

/* ---- scoring: per-token log-probs, rank, KL against a second set of logits and the top-k log-probs, one launch ----------------
 * logits fp16 [N, V] with a row pitch ld >= V (elements); ids int64 [N] = the target token of each row; ref_logits (optional):
 * a second fp16 matrix of the same shape and pitch, the other cache's logits for the same tokens; k_top in [0, 8].
 * Outputs (each may be NULL, except lp):
 *   lp      fp32  [N]        logits[i, ids[i]] - logsumexp(logits[i, :])
 *   lse     fp32  [N]        the log-sum-exp
 *   rank    int32 [N]        entries strictly greater than the target's logit (0 = the target is the argmax)
 *   kl      fp32  [N]        KL(softmax(ref_logits[i]) || softmax(logits[i])) in nats            (needs ref_logits)
 *   agree   int32 [N]        1 where both rows have the same argmax (equal values: lowest index) (needs ref_logits)
 *   top_idx int32 [N, k_top], top_lp fp32 [N, k_top]   the k_top largest log-probs, descending; equal values by index, lowest first
 * Semantics:
 *   - one workgroup per row (rows ride on gridDim.x: N may exceed 65535); a row is never split over workgroups, the workgroup
 *     size is a function of V alone and every merge runs in a fixed order: a row's results depend on that row's contents only,
 *     not on N or on the row's position, and the same call on the same data gives the same bits;
 *   - one streaming pass with a running maximum: the statistics are fp32 sums of exp(x - max), so logits up to fp16's largest
 *     value cannot overflow; the final log / subtraction run in fp64 and are rounded once.  k_top > 1 re-reads the row
 *     k_top - 1 times (cache-resident: the workgroup has just read it);
 *   - -inf logits (a masked vocabulary entry) contribute 0 to the sum; a target whose logit is -inf gives lp = -inf; a row that
 *     is all -inf gives NaN in lp, lse (and kl, top_lp);
 *   - ids[i] < 0 marks an ignored row (HF's -100): lp = 0, rank = -1; ids[i] >= V gives lp = NaN, rank = -1; neither indexes a read;
 *   - kl = sum_j p_j (ref_j - x_j) - lse(ref) + lse(x): an entry with ref_j = -inf contributes 0, an entry with x_j = -inf under a
 *     finite ref_j makes it +inf;
 *   - loads are 16 bytes wide when a row (and its ref_logits row) starts on a 16-byte boundary; a row that does not (an odd ld, a
 *     sliced view) is read with the widest loads its 2-byte alignment allows -- the same columns in the same order, so the bits do
 *     not depend on where a row lies.  The V % 8 columns behind the last whole vector are read one by one.  Nothing past column
 *     V - 1 of a row is read;
 * Refused with a status < 0 and a gear_last_error message before any launch: null logits / ids / lp, V <= 0, N < 0 (or > 2^31 - 1),
 * ld < V, k_top outside [0, 8] or > V, kl or agree without ref_logits.  N == 0 returns 0 without a launch. */
int gear_token_logprobs(const void* logits, const void* ref_logits, const int64_t* ids, int64_t N, int V, int64_t ld, int k_top,
                        float* lp, float* lse, int32_t* rank, float* kl, int32_t* agree, int32_t* top_idx, float* top_lp,
                        void* stream);

/* ---- logits processors and EOS bookkeeping for the decoders (csrc/logits.hip) -------------------------------------------------
 * What HF's generate() applies between lm_head and the token choice (the reference evaluates through it:
 * GenerationBench/GenerationTest/evaluation_bbh_cot.py:374-392), as ONE launch per step with one workgroup per row.  Neither
 * entry point synchronises or allocates: both are graph-capturable.
 *
 * The processing launch:
 *   logits  fp16 [B, V] (fp32 when logits_fp32), row pitch ld >= V elements; 1 <= V <= 262144
 *   out     the same type, row pitch ld_out >= V; may be the very pointer `logits` (with ld_out == ld), never a partial overlap
 *   hist    int32 [B, hist_cap]: prompt + generated tokens of every sequence; the live length is n = pos0 + *pos_dev (pos_dev: a
 *           device int32, e.g. the decode state {pos, ...}; NULL: n = pos0), clamped to [0, hist_cap]
 *   cur     optional int64 [B]: the token just fed.  It is stored at hist[b][n - 1] by one lane (a plain vector store) in front of a
 *           workgroup barrier, and the launch itself reads entry n - 1 from cur: the history grows inside a captured step
 *   prompt_len  length of the prompt part of the history (min_new_tokens counts n - prompt_len)
 *   params  (host pointer) repetition_penalty > 0 (1: off), no_repeat_ngram >= 0 (0: off), min_new_tokens >= 0, n_eos <= 8 EOS ids
 *           inline, n_bias pairs {int32 token, float bias} in DEVICE memory with unique tokens (a bias of -inf is a ban)
 * Per row, in HF's processor order, with x_j = fp32(logits[j]):
 *   1. bias     x_t += bias for every pair (SequenceBiasLogitsProcessor with length-1 sequences)
 *   2. penalty  once for every distinct token of hist[b][0 .. n): x < 0 ? x * p : x / p (RepetitionPenaltyLogitsProcessor) -- the
 *               history marks an LDS bitmap of V bits with atomicOr, so duplicates cannot apply it twice
 *   3. bans     x = -inf: with g = no_repeat_ngram and n >= g, hist[i + g - 1] for every i whose g - 1 tokens hist[i .. i + g - 1)
 *               equal the last g - 1 tokens hist[n - g + 1 .. n) (NoRepeatNGramLogitsProcessor; g = 1 bans every seen token);
 *               every EOS id while n - prompt_len < min_new_tokens (MinNewTokensLengthLogitsProcessor)
 * out[j] = the value rounded ONCE to the output type (fp32 arithmetic, IEEE division).  An entry no processor touches comes out
 * with the bits it came in with (also -0, NaN payloads); -inf stays -inf.  History, EOS and bias ids outside [0, V) are skipped and
 * never index anything.  Nothing is read or written past column V - 1 of a row or past entry n - 1 of a history.  Rows that start
 * on a 16-byte boundary (input and output) move in 16-byte vectors, other rows (an odd pitch, a sliced view) in the widest
 * accesses their alignment allows -- the same bits either way.
 * Refused with a status < 0 and a gear_last_error message before any launch: null logits / out / hist / params, V <= 0 or
 * V > 262144, ld < V or ld_out < V, B < 0, a penalty that is <= 0 or NaN, no_repeat_ngram < 0, min_new_tokens < 0, n_eos outside
 * [0, 8], n_bias < 0 or n_bias > 0 with a null table, pos0 < 0, hist_cap <= 0.  B == 0 returns 0 without a launch.
 *
 * The EOS launch (after the token choice): tok int64 [B] and done int32 [B] are read and written -- a row with done[b] != 0 gets
 * tok[b] = pad; otherwise, if tok[b] is one of the n_eos <= 8 ids (host array), done[b] = 1 and the EOS token itself stays.
 * *n_done (device int32) = the number of rows with done != 0 after the update (integer sums, merged in wave order).  One
 * workgroup.  Refused: null tok / done / n_done, B < 0, n_eos outside [0, 8], n_eos > 0 with null ids; B == 0 returns 0. */
typedef struct {
    float repetition_penalty;
    int no_repeat_ngram;
    int min_new_tokens;
    int n_eos;
    int eos[8];
    int n_bias;
    int reserved;
    const void* bias;
} gear_logits_params;
int gear_logits_process(const void* logits, void* out, int logits_fp32, int B, int V, int64_t ld, int64_t ld_out, int32_t* hist,
                        int hist_cap, const int* pos_dev, int pos0, const int64_t* cur, int prompt_len,
                        const gear_logits_params* p, void* stream);
int gear_eos_update(int64_t* tok, int32_t* done, int B, const int* eos, int n_eos, int64_t pad, int32_t* n_done, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEAR_HIP_H */
