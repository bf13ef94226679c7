// Every function that crosses a translation-unit boundary, declared once.
// bindings.hip (the only caller) and the defining .hip file both include this
// header, so a definition that disagrees with its declaration does not compile.
//
// Each launcher owns its kernel's grid, block and LDS arithmetic and launches
// on `stream`. The one-line contracts below are what the CALLER guarantees;
// bindings.hip checks all of it on the host before it calls. What lives on the
// device stays the caller's contract and is checked nowhere on the host:
// positions below the cos/sin table length, slots inside the cache, block ids
// below NB, context lengths within the block table, pair indices below N.
// Unless a contract says otherwise a launcher is not called with zero rows.
#pragma once

#include "common.h"

// decode-attention partials: [B, KVH, max_chunks, gqa, ATTN_DECODE_PART_STRIDE]
// fp32, 128 unnormalised o values, then m, then l
#define ATTN_DECODE_PART_STRIDE 130

static inline int64_t attn_decode_partials_numel(int B, int num_q_heads, int max_chunks) {
  return (int64_t)B * num_q_heads * max_chunks * ATTN_DECODE_PART_STRIDE;
}

extern "C" {

// --- elementwise.hip ---
// out/in [rows, n] dense bf16, w [n]; n % 8 == 0, all 16-byte aligned.
void launch_rmsnorm(bf16_t* out, const bf16_t* in, const bf16_t* w, int rows, int n, float eps,
                    hipStream_t stream);
// residual += x in place, out = rmsnorm(residual); shapes and alignment as launch_rmsnorm.
void launch_fused_add_rmsnorm(bf16_t* out, const bf16_t* x, bf16_t* residual, const bf16_t* w,
                              int rows, int n, float eps, hipStream_t stream);
// out [rows, ncols] dense; gate/up [rows, ncols] with row stride `row_stride` elements;
// ncols % 8 == 0, row_stride % 8 == 0, all three bases 16-byte aligned.
void launch_silu_mul(bf16_t* out, const bf16_t* gate, const bf16_t* up, int64_t rows,
                     int64_t ncols, int64_t row_stride, hipStream_t stream);
// q [T, H, D] / k [T, KVH, D] row views (token strides in elements), positions [T],
// cos_sin [max_pos, D]; D even, D / 2 <= 1024.
void launch_rope(bf16_t* q, bf16_t* k, const int64_t* positions, const float* cos_sin, int T,
                 int num_q_heads, int num_kv_heads, int head_dim, int q_tstride, int k_tstride,
                 hipStream_t stream);
// k/v [T, KVH, D] row views sharing kv_tstride, caches [NB, KVH, BS, D], slots [T];
// cache_fp8: e4m3 caches and k_scale/v_scale [NB, KVH, BS] (else bf16 caches, scales
// unused); bf16 needs D % 8 == 0 and 16-byte-aligned k/v rows.
void launch_store_kv(const bf16_t* k, const bf16_t* v, void* k_cache, void* v_cache,
                     float* k_scale, float* v_scale, const int64_t* slots, int T,
                     int num_kv_heads, int head_dim, int block_size, int kv_tstride,
                     int cache_fp8, hipStream_t stream);
// launch_rope on q/k, then launch_store_kv of the rotated k and v, in one kernel;
// D % 8 == 0 and v rows 16-byte aligned.
void launch_rope_store_kv(bf16_t* q, bf16_t* k, const bf16_t* v, void* k_cache, void* v_cache,
                          float* k_scale, float* v_scale, const int64_t* positions,
                          const float* cos_sin, const int64_t* slots, int T, int num_q_heads,
                          int num_kv_heads, int head_dim, int block_size, int q_tstride,
                          int k_tstride, int v_tstride, int cache_fp8, hipStream_t stream);

// --- kv_copy.hip ---
// src/dst [n_pairs] block ids; vec_bytes (16, 4 or 1) divides both bases, layer_stride
// and block_bytes; zero pairs or layers is a no-op.
void launch_copy_kv_blocks(void* a_base, void* b_base, const int* src, const int* dst,
                           int n_pairs, int n_layers, int64_t layer_stride,
                           int64_t block_bytes, int vec_bytes, hipStream_t stream);

// --- attn_decode.hip ---
// partials of attn_decode_partials_numel(B, H, max_chunks) floats; q [B, H, 128] with
// row stride q_tstride; caches [NB, KVH, BS, 128]; block_tables [B, max_blocks];
// context_lens [B]; skip_chunks [B] or null; H / KVH in {1, 2, 4, 8}; scales non-null
// iff cache_fp8.
void launch_attn_decode_partial(float* partials, const bf16_t* q, const void* k_cache,
                                const void* v_cache, const float* k_scale, const float* v_scale,
                                const int* block_tables, const int* context_lens,
                                const int* skip_chunks, float scale, int num_q_heads,
                                int num_kv_heads, int block_size, int max_blocks, int max_chunks,
                                int q_tstride, int chunk_keys, int B, int cache_fp8,
                                hipStream_t stream);
// out [B, H, 128] dense; merges the partials launch_attn_decode_partial (and _shared) wrote.
void launch_attn_decode_reduce(bf16_t* out, const float* partials, const int* context_lens,
                               int B, int num_q_heads, int num_kv_heads, int max_chunks,
                               int chunk_keys, hipStream_t stream);

// --- attn_decode_shared.hip ---
// as launch_attn_decode_partial, plus tile_rows [n_tiles, 64], tile_nmembers [n_tiles],
// tile_chunks [n_tiles]; zero tiles is a no-op.
void launch_attn_decode_shared(float* partials, const bf16_t* q, const void* k_cache,
                               const void* v_cache, const float* k_scale, const float* v_scale,
                               const int* block_tables, const int* tile_rows,
                               const int* tile_nmembers, const int* tile_chunks, float scale,
                               int B, int num_q_heads, int num_kv_heads, int num_blocks,
                               int block_size, int max_blocks, int max_chunks, int q_tstride,
                               int n_tiles, int cache_fp8, hipStream_t stream);

// --- attn_prefill.hip ---
// out [T, H, 128] dense; q [T, H, 128], k/v [T, KVH, 128] row views with 16-byte rows
// (k and v share kv_tstride); grp_seq_start / grp_seqlen [n_groups], grp_qpos0
// [n_groups * 8]; H % KVH == 0.
void launch_attn_prefill(bf16_t* out, const bf16_t* q, const bf16_t* k, const bf16_t* v,
                         const int* grp_seq_start, const int* grp_seqlen, const int* grp_qpos0,
                         float scale, int n_groups, int num_q_heads, int num_kv_heads,
                         int q_tstride, int kv_tstride, hipStream_t stream);

// --- attn_prefill_paged.hip ---
// out [total_rows, H, 128] dense; q the same with row stride q_tstride, 16-byte rows;
// caches [num_blocks, KVH, BS, 128]; block_tables [n_seq, max_blocks]; cu_q [n_seq + 1];
// q_start [n_seq]; grp_seq [n_groups]; grp_qpos0 [n_groups * 8]; scales non-null iff
// cache_fp8; an empty grid is a no-op.
void launch_attn_prefill_paged(bf16_t* out, const bf16_t* q, const void* k_cache,
                               const void* v_cache, const float* k_scale, const float* v_scale,
                               const int* block_tables, const int* cu_q, const int* q_start,
                               const int* grp_seq, const int* grp_qpos0, float scale, int n_seq,
                               int total_rows, int num_q_heads, int num_kv_heads,
                               int num_blocks, int block_size, int max_blocks, int q_tstride,
                               int n_groups, int cache_fp8, hipStream_t stream);
// as launch_attn_prefill_paged, plus grp_krange [n_groups * 2], grp_split [n_groups],
// seq_nsplit / seq_ws_base [n_seq], part_o [>= ws_rows, H, 128] and part_ml
// [>= ws_rows, H, 2] fp32, 16-byte aligned; 2 <= max_splits <= 64.
void launch_attn_prefill_paged_split(
    bf16_t* out, const bf16_t* q, const void* k_cache, const void* v_cache,
    const float* k_scale, const float* v_scale, const int* block_tables, const int* cu_q,
    const int* q_start, const int* grp_seq, const int* grp_qpos0, const int* grp_krange,
    const int* grp_split, const int* seq_nsplit, const int* seq_ws_base, float* part_o,
    float* part_ml, int ws_rows, int max_splits, float scale, int n_seq, int total_rows,
    int num_q_heads, int num_kv_heads, int num_blocks, int block_size, int max_blocks,
    int q_tstride, int n_groups, int cache_fp8, hipStream_t stream);

// --- sampling.hip ---
// tokens / logprobs and the five per-row parameters [B]; logits [B, V] dense fp32;
// mask [B, ceil(V / 32)] words or null; dbg [B, 16] or null.
void launch_sample(int64_t* tokens, float* logprobs, const float* logits,
                   const float* temperatures, const float* top_ps, const int* top_ks,
                   const int64_t* seeds, const int64_t* steps, const uint32_t* mask, int B, int V,
                   float* dbg, hipStream_t stream);
// as launch_sample without mask/dbg; fsm_state [B] (advanced in place), tabs [B, 6]
// device addresses of tables the caller keeps alive; -1 <= eos_id < V.
void launch_sample_fsm(int64_t* tokens, float* logprobs, const float* logits,
                       const float* temperatures, const float* top_ps, const int* top_ks,
                       const int64_t* seeds, const int64_t* steps, int32_t* fsm_state,
                       const int64_t* tabs, int eos_id, int B, int V, hipStream_t stream);

// --- mfma_selftest.hip ---
// D [32, 32] fp32 = A [32, 16] x B [16, 32], dense bf16.
void launch_mfma_selftest(float* D, const bf16_t* A, const bf16_t* B, hipStream_t stream);

// --- allreduce.hip ---
// srcs/dsts: n_peers (1..8) host arrays of device bf16 buffers of numel elements;
// numel % 8 == 0, 16-byte-aligned buffers, all reachable from the current device.
void launch_one_shot_allreduce(const void* const* srcs, void* const* dsts, int n_peers,
                               long numel, int write_all, hipStream_t stream);
// 1 <= world <= 8; handles_out takes 128 bytes; returns null on failure.
void* ipc_ar_create(int rank, int world, size_t max_bytes, unsigned char* handles_out);
// all_handles: world * 128 bytes, every rank's ipc_ar_create output in rank order.
int ipc_ar_connect(void* ctx, const unsigned char* all_handles);
// inp/out: numel bf16 on ctx's device; refuses (-2) numel % 8 != 0 or more than max_bytes.
int ipc_ar_run(void* ctx, const void* inp, void* out, long numel, hipStream_t stream);
// ctx from ipc_ar_create, or null.
void ipc_ar_destroy(void* ctx);

// --- moe.hip ---
// act [S, IN], x [T, K] dense bf16; w [E, 2 * IN, K] bf16 (scale null) or e4m3 with
// scale [E, 2 * IN]; sorted_ids [S]; pad_offsets [E + 1]; zeros [>= K]; S % 128 == 0,
// IN % 64 == 0, K % 64 == 0.
void launch_moe_gateup(void* act, const void* x, const void* w, const float* scale,
                       const int* sorted_ids, const int* pad_offsets, const void* zeros, int E,
                       int IN, int K, hipStream_t stream);
// y [S, H], act [S, IN] dense bf16; w [E, H, IN] and scale [E, H] as launch_moe_gateup;
// pad_offsets [E + 1]; H % 64 == 0, IN % 64 == 0.
void launch_moe_down(void* y, const void* act, const void* w, const float* scale,
                     const int* pad_offsets, int E, int H, int IN, hipStream_t stream);

// --- levenshtein.hip ---
// out / pi / pj [n_pairs]; chars [N, 64] dense; lens [N], each <= 64.
void launch_levenshtein(int* out, const unsigned char* chars, const int* lens, const int* pi,
                        const int* pj, long n_pairs, hipStream_t stream);

// --- linear_fp8w.hip ---
// pure function of the shape and CU count; writes the row tile and split-K to use.
void linear_fp8w_plan(int M, int N, int K, int n_cus, int* mt, int* splitk);
// the same for E problems in one launch.
void linear_fp8w_batched_plan(int E, int M, int N, int K, int n_cus, int* mt, int* splitk);
// out [M, N] bf16; x [M, K] bf16 rows of stride x_stride (16-byte rows); q [N, K] e4m3,
// scale [N], both 16-byte aligned; bias [N] or null; slabs [splitk, M, N] fp32 iff
// splitk > 1; mt/splitk from linear_fp8w_plan; 1 <= M <= 256, K % 64 == 0, N % 16 == 0.
void launch_linear_fp8w(void* out, float* slabs, const void* x, const void* q,
                        const float* scale, const void* bias, int M, int N, int K,
                        long x_stride, int mt, int splitk, hipStream_t stream);
// out [E, M, N]; q [E, N, K]; scale [E, N]; x rows of stride x_stride, experts of stride
// x_bstride (0: one x for all); slabs [E, splitk, M, N] iff splitk > 1; limits as above.
void launch_linear_fp8w_batched(void* out, float* slabs, const void* x, const void* q,
                                const float* scale, int E, int M, int N, int K, long x_stride,
                                long x_bstride, int mt, int splitk, hipStream_t stream);
// w [numel] bf16 = q [numel / K, K] e4m3 * scale per row; K % 16 == 0, 16-byte aligned.
void launch_dequant_fp8w(void* w, const void* q, const float* scale, long numel, int K,
                         hipStream_t stream);

}  // extern "C"
