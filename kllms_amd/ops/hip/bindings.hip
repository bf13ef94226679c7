// PyTorch bindings for the kllms_amd gfx950 kernels (kllms_amd._C).
// Thin launch shims: shape/dtype checks, grid math, current-HIP-stream launch.

#include <algorithm>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

// kernels (defined in the sibling .hip TUs)
extern "C" __global__ void rmsnorm_kernel(bf16_t*, const bf16_t*, const bf16_t*, int, float);
extern "C" __global__ void fused_add_rmsnorm_kernel(bf16_t*, const bf16_t*, bf16_t*, const bf16_t*, int, float);
extern "C" __global__ void silu_mul_kernel(bf16_t*, const bf16_t*, const bf16_t*, int64_t, int, int);
extern "C" __global__ void rope_kernel(bf16_t*, bf16_t*, const int64_t*, const float*, int, int, int, int, int);
extern "C" __global__ void store_kv_kernel(const bf16_t*, const bf16_t*, bf16_t*, bf16_t*, const int64_t*, int, int, int, int, int);
extern "C" __global__ void store_kv_fp8_kernel(const bf16_t*, const bf16_t*, unsigned char*, unsigned char*, float*, float*, const int64_t*, int, int, int, int, int);
extern "C" __global__ void rope_store_kv_kernel(bf16_t*, bf16_t*, const bf16_t*, bf16_t*, bf16_t*, const int64_t*, const float*, const int64_t*, int, int, int, int, int, int, int);
extern "C" __global__ void rope_store_kv_fp8_kernel(bf16_t*, bf16_t*, const bf16_t*, unsigned char*, unsigned char*, float*, float*, const int64_t*, const float*, const int64_t*, int, int, int, int, int, int, int);
extern "C" void launch_copy_kv_blocks(void*, void*, const int*, const int*, int, int, int64_t, int64_t, int, hipStream_t);
extern "C" void launch_attn_decode_partial(float*, const bf16_t*, const void*, const void*, const float*, const float*, const int*, const int*, const int*, float, int, int, int, int, int, int, int, int, int, hipStream_t);
extern "C" void launch_attn_decode_shared(float*, const bf16_t*, const void*, const void*, const float*, const float*, const int*, const int*, const int*, const int*, float, int, int, int, int, int, int, int, int, int, int, hipStream_t);
extern "C" void launch_attn_prefill_paged(bf16_t*, const bf16_t*, const void*, const void*, const float*, const float*, const int*, const int*, const int*, const int*, const int*, float, int, int, int, int, int, int, int, int, int, int, hipStream_t);
extern "C" void launch_attn_prefill_paged_split(bf16_t*, const bf16_t*, const void*, const void*, const float*, const float*, const int*, const int*, const int*, const int*, const int*, const int*, const int*, const int*, const int*, float*, float*, int, int, float, int, int, int, int, int, int, int, int, int, int, hipStream_t);
extern "C" __global__ void attn_decode_reduce_kernel(bf16_t*, const float*, const int*, int, int, int, int);
extern "C" __global__ void attn_prefill_kernel(bf16_t*, const bf16_t*, const bf16_t*, const bf16_t*, const int*, const int*, const int*, float, int, int, int, int);  // grouped: [G], [G], [G*8]
extern "C" __global__ void sample_kernel(int64_t*, float*, const float*, const float*, const float*, const int*, const int64_t*, const int64_t*, const uint32_t*, int, float*);
extern "C" __global__ void sample_fsm_kernel(int64_t*, float*, const float*, const float*, const float*, const int*, const int64_t*, const int64_t*, int32_t*, const int64_t*, int, int);
extern "C" __global__ void mfma_selftest_kernel(float*, const bf16_t*, const bf16_t*);

#define CHECK_BF16_CONTIG(t) \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous() && (t).scalar_type() == at::kBFloat16, #t " must be contiguous bf16 on GPU")

// [T, H, D] activation views: head/dim dims packed, token stride free (so the
// fused-QKV splits need no .contiguous() copies)
#define CHECK_KV_CACHE(t) \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous() && \
              ((t).scalar_type() == at::kBFloat16 || (t).scalar_type() == at::kFloat8_e4m3fn), \
              #t " must be a contiguous bf16 or fp8-e4m3 KV cache on GPU")

#define CHECK_BF16_ROWS(t) \
  TORCH_CHECK((t).is_cuda() && (t).scalar_type() == at::kBFloat16 && (t).dim() == 3 && \
              (t).stride(2) == 1 && (t).stride(1) == (t).size(2), #t " must be a bf16 [T,H,D] row view")

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

static bf16_t* bf(torch::Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }
static const bf16_t* cbf(const torch::Tensor& t) { return reinterpret_cast<const bf16_t*>(t.data_ptr()); }

void rmsnorm(torch::Tensor out, torch::Tensor in, torch::Tensor weight, double eps) {
  CHECK_BF16_CONTIG(out); CHECK_BF16_CONTIG(in); CHECK_BF16_CONTIG(weight);
  const int n = in.size(-1);
  TORCH_CHECK(n % 8 == 0, "hidden size must be a multiple of 8");
  const int rows = in.numel() / n;
  hipLaunchKernelGGL(rmsnorm_kernel, dim3(rows), dim3(256), 0, cur_stream(),
                     bf(out), cbf(in), cbf(weight), n, (float)eps);
}

void fused_add_rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor residual,
                       torch::Tensor weight, double eps) {
  CHECK_BF16_CONTIG(out); CHECK_BF16_CONTIG(x); CHECK_BF16_CONTIG(residual); CHECK_BF16_CONTIG(weight);
  const int n = x.size(-1);
  TORCH_CHECK(n % 8 == 0, "hidden size must be a multiple of 8");
  const int rows = x.numel() / n;
  hipLaunchKernelGGL(fused_add_rmsnorm_kernel, dim3(rows), dim3(256), 0, cur_stream(),
                     bf(out), cbf(x), bf(residual), cbf(weight), n, (float)eps);
}

void silu_mul(torch::Tensor out, torch::Tensor gate, torch::Tensor up) {
  CHECK_BF16_CONTIG(out);
  TORCH_CHECK(gate.is_cuda() && gate.scalar_type() == at::kBFloat16 && gate.dim() == 2 &&
              gate.stride(1) == 1, "gate must be a bf16 [T, I] row view");
  TORCH_CHECK(up.sizes() == gate.sizes() && up.stride(0) == gate.stride(0) && up.stride(1) == 1);
  const int64_t ncols = gate.size(1);
  TORCH_CHECK(ncols % 8 == 0 && gate.stride(0) % 8 == 0);
  const int64_t nvec = gate.numel() / 8;
  const int grid = (int)std::min<int64_t>((nvec + 255) / 256, 2048);
  hipLaunchKernelGGL(silu_mul_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                     bf(out), cbf(gate), cbf(up), nvec, (int)(ncols / 8), (int)(gate.stride(0) / 8));
}

void rope_inplace(torch::Tensor q, torch::Tensor k, torch::Tensor positions, torch::Tensor cos_sin) {
  CHECK_BF16_ROWS(q); CHECK_BF16_ROWS(k);
  TORCH_CHECK(positions.scalar_type() == at::kLong && cos_sin.scalar_type() == at::kFloat);
  const int T = q.size(0), H = q.size(1), D = q.size(2), KVH = k.size(1);
  hipLaunchKernelGGL(rope_kernel, dim3(T, H + KVH), dim3(D / 2), 0, cur_stream(),
                     bf(q), bf(k), positions.data_ptr<int64_t>(), cos_sin.data_ptr<float>(),
                     H, KVH, D, (int)q.stride(0), (int)k.stride(0));
}

void store_kv(torch::Tensor k, torch::Tensor v, torch::Tensor k_cache, torch::Tensor v_cache,
              torch::Tensor slot_mapping, torch::Tensor k_scale, torch::Tensor v_scale) {
  CHECK_BF16_ROWS(k); CHECK_BF16_ROWS(v); CHECK_KV_CACHE(k_cache); CHECK_KV_CACHE(v_cache);
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v must share the token stride");
  const int T = k.size(0), KVH = k.size(1), D = k.size(2);
  const int BS = k_cache.size(2);
  if (k_cache.scalar_type() == at::kFloat8_e4m3fn) {
    // per-row quantization: one wave per (token, head) row, 4 waves/block
    TORCH_CHECK(k_scale.numel() == k_cache.size(0) * KVH * BS && k_scale.is_contiguous() &&
                    k_scale.scalar_type() == at::kFloat && v_scale.numel() == k_scale.numel(),
                "fp8 store_kv requires [NB, KVH, BS] fp32 k_scale/v_scale");
    const int64_t rows = (int64_t)T * KVH;
    const int grid = (int)std::min<int64_t>((rows + 3) / 4, 2048);
    hipLaunchKernelGGL(store_kv_fp8_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                       cbf(k), cbf(v),
                       reinterpret_cast<unsigned char*>(k_cache.data_ptr()),
                       reinterpret_cast<unsigned char*>(v_cache.data_ptr()),
                       k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),
                       slot_mapping.data_ptr<int64_t>(), T, KVH, D, BS, (int)k.stride(0));
  } else {
    const int64_t total = (int64_t)T * KVH * (D / 8);
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(store_kv_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                       cbf(k), cbf(v), bf(k_cache), bf(v_cache),
                       slot_mapping.data_ptr<int64_t>(), T, KVH, D, BS, (int)k.stride(0));
  }
}

// rope_inplace + store_kv in one launch (elementwise.hip): q/k rotated in
// place, the rotated k and the untouched v scattered to the paged caches at
// slot_mapping. Same views and the same bits as the two separate ops.
void rope_store_kv(torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor positions,
                   torch::Tensor cos_sin, torch::Tensor k_cache, torch::Tensor v_cache,
                   torch::Tensor slot_mapping, torch::Tensor k_scale, torch::Tensor v_scale) {
  CHECK_BF16_ROWS(q); CHECK_BF16_ROWS(k); CHECK_BF16_ROWS(v);
  CHECK_KV_CACHE(k_cache); CHECK_KV_CACHE(v_cache);
  TORCH_CHECK(positions.is_cuda() && positions.scalar_type() == at::kLong && positions.is_contiguous() &&
              cos_sin.is_cuda() && cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous(),
              "rope_store_kv: positions must be int64 and cos_sin fp32, contiguous on GPU");
  TORCH_CHECK(slot_mapping.is_cuda() && slot_mapping.scalar_type() == at::kLong &&
              slot_mapping.is_contiguous(), "rope_store_kv: slot_mapping must be contiguous int64 on GPU");
  const int T = q.size(0), H = q.size(1), D = q.size(2), KVH = k.size(1);
  TORCH_CHECK(k.size(0) == T && v.size(0) == T && k.size(2) == D && v.size(2) == D &&
              v.size(1) == KVH, "rope_store_kv: q/k/v disagree on T, KVH or D");
  TORCH_CHECK(positions.numel() == T && slot_mapping.numel() == T,
              "rope_store_kv: positions and slot_mapping must be [T]");
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() &&
              v_cache.scalar_type() == k_cache.scalar_type() && k_cache.size(1) == KVH &&
              k_cache.size(3) == D && cos_sin.size(-1) == D,
              "rope_store_kv: caches must be [NB, KVH, BS, D] of one dtype, cos_sin [max_pos, D]");
  TORCH_CHECK(D % 8 == 0 && v.stride(0) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0,
              "rope_store_kv: head_dim must be a multiple of 8 and v rows 16-byte aligned");
  if (T == 0) return;
  const int BS = k_cache.size(2);
  const dim3 grid(T, (H + KVH + 3) / 4);
  if (k_cache.scalar_type() == at::kFloat8_e4m3fn) {
    TORCH_CHECK(k_scale.is_cuda() && v_scale.is_cuda() &&
                    k_scale.numel() == k_cache.size(0) * KVH * BS && k_scale.is_contiguous() &&
                    v_scale.is_contiguous() && k_scale.scalar_type() == at::kFloat &&
                    v_scale.scalar_type() == at::kFloat && v_scale.numel() == k_scale.numel(),
                "fp8 rope_store_kv requires [NB, KVH, BS] fp32 k_scale/v_scale");
    hipLaunchKernelGGL(rope_store_kv_fp8_kernel, grid, dim3(256), 0, cur_stream(),
                       bf(q), bf(k), cbf(v),
                       reinterpret_cast<unsigned char*>(k_cache.data_ptr()),
                       reinterpret_cast<unsigned char*>(v_cache.data_ptr()),
                       k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),
                       positions.data_ptr<int64_t>(), cos_sin.data_ptr<float>(),
                       slot_mapping.data_ptr<int64_t>(), H, KVH, D, BS,
                       (int)q.stride(0), (int)k.stride(0), (int)v.stride(0));
  } else {
    hipLaunchKernelGGL(rope_store_kv_kernel, grid, dim3(256), 0, cur_stream(),
                       bf(q), bf(k), cbf(v), bf(k_cache), bf(v_cache),
                       positions.data_ptr<int64_t>(), cos_sin.data_ptr<float>(),
                       slot_mapping.data_ptr<int64_t>(), H, KVH, D, BS,
                       (int)q.stride(0), (int)k.stride(0), (int)v.stride(0));
  }
}

// Copy blocks src[i] -> dst[i] of the two [L, NB, ...] arrays `a` and `b` (K
// and V, or the two fp8 scale arrays) for every layer in one launch
// (kv_copy.hip). src/dst: int32 [n] on the GPU, validated by the caller
// (in range, no block both a source and a destination).
void copy_kv_blocks(torch::Tensor a, torch::Tensor b, torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.is_contiguous() && b.is_contiguous() &&
              a.dim() >= 2 && a.sizes() == b.sizes() && a.scalar_type() == b.scalar_type(),
              "copy_kv_blocks: a/b must be contiguous [L, NB, ...] GPU arrays of one shape and dtype");
  auto ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == a.device() && t.is_contiguous() &&
           t.scalar_type() == at::kInt && t.dim() == 1;
  };
  TORCH_CHECK(ok(src) && ok(dst) && src.numel() == dst.numel(),
              "copy_kv_blocks: src/dst must be contiguous int32 [n] on the arrays' device");
  const int64_t n = src.numel(), L = a.size(0), NB = a.size(1);
  if (n == 0 || L == 0 || NB == 0) return;
  TORCH_CHECK(n <= INT32_MAX / 2 / L, "copy_kv_blocks: too many pairs");
  const int64_t block_bytes = a.stride(1) * (int64_t)a.element_size();
  const int64_t layer_stride = a.stride(0) * (int64_t)a.element_size();
  const uintptr_t bits = reinterpret_cast<uintptr_t>(a.data_ptr()) |
                         reinterpret_cast<uintptr_t>(b.data_ptr()) |
                         (uintptr_t)block_bytes | (uintptr_t)layer_stride;
  const int vec = bits % 16 == 0 ? 16 : (bits % 4 == 0 ? 4 : 1);
  launch_copy_kv_blocks(a.data_ptr(), b.data_ptr(), src.data_ptr<int>(), dst.data_ptr<int>(),
                        (int)n, (int)L, layer_stride, block_bytes, vec, cur_stream());
}

// Shared body of the two decode-attention bindings. With `shared` false this
// is exactly the per-stream split-K path; with it true the shared-prefix
// kernel first writes the partials of each group's leading chunks and the
// per-stream kernel skips them (skip_chunks). The reduce is the same.
static void attn_decode_paged_impl(torch::Tensor& out, torch::Tensor& q, torch::Tensor& k_cache,
                                   torch::Tensor& v_cache, torch::Tensor& block_tables,
                                   torch::Tensor& context_lens, double scale,
                                   torch::Tensor& k_scale, torch::Tensor& v_scale, bool shared,
                                   const int* skip_chunks, const int* tile_rows,
                                   const int* tile_nmembers, const int* tile_chunks,
                                   int n_tiles) {
  CHECK_BF16_CONTIG(out); CHECK_BF16_ROWS(q); CHECK_KV_CACHE(k_cache); CHECK_KV_CACHE(v_cache);
  const int B = q.size(0), H = q.size(1), D = q.size(2);
  const int KVH = k_cache.size(1), BS = k_cache.size(2);
  TORCH_CHECK(D == 128, "attn_decode: head_dim must be 128");
  TORCH_CHECK(H % KVH == 0, "attn_decode: H must be a multiple of KVH");
  TORCH_CHECK(H / KVH == 1 || H / KVH == 2 || H / KVH == 4 || H / KVH == 8,
              "attn_decode: GQA group must be 1, 2, 4 or 8");
  const int gqa = H / KVH;
  const int max_blocks = block_tables.size(1);
  // split-K granule: fixed 256 keys measured best across B=40..240 and
  // ctx 576..2048 (adaptive coarser chunks trade combine traffic for lost
  // block-level parallelism and net 0..-5%; chunk size stays a runtime arg)
  const int max_ctx = max_blocks * BS;
  const int CHUNK_KEYS = ATTN_DECODE_TKV;  // 256
  const int max_chunks = std::max(1, (max_ctx + CHUNK_KEYS - 1) / CHUNK_KEYS);
  auto partials = torch::empty({(int64_t)B * KVH * max_chunks * gqa * 130},
                               torch::dtype(torch::kFloat).device(q.device()));
  const int cache_fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn ? 1 : 0;
  if (cache_fp8) {
    TORCH_CHECK(k_scale.numel() == k_cache.size(0) * KVH * BS && k_scale.is_contiguous() &&
                    k_scale.scalar_type() == at::kFloat && v_scale.numel() == k_scale.numel(),
                "fp8 attn_decode requires [NB, KVH, BS] fp32 k_scale/v_scale");
  }
  if (shared && n_tiles > 0) {
    launch_attn_decode_shared(
        partials.data_ptr<float>(), cbf(q), k_cache.data_ptr(), v_cache.data_ptr(),
        cache_fp8 ? k_scale.data_ptr<float>() : nullptr,
        cache_fp8 ? v_scale.data_ptr<float>() : nullptr,
        block_tables.data_ptr<int>(), tile_rows, tile_nmembers, tile_chunks,
        (float)scale, B, H, KVH, (int)k_cache.size(0), BS, max_blocks, max_chunks,
        (int)q.stride(0), n_tiles, cache_fp8, cur_stream());
  }
  launch_attn_decode_partial(
      partials.data_ptr<float>(), cbf(q), k_cache.data_ptr(), v_cache.data_ptr(),
      cache_fp8 ? k_scale.data_ptr<float>() : nullptr,
      cache_fp8 ? v_scale.data_ptr<float>() : nullptr,
      block_tables.data_ptr<int>(), context_lens.data_ptr<int>(),
      (shared && n_tiles > 0) ? skip_chunks : nullptr,
      (float)scale, H, KVH, BS, max_blocks, max_chunks, (int)q.stride(0), CHUNK_KEYS, B,
      cache_fp8, cur_stream());
  hipLaunchKernelGGL(attn_decode_reduce_kernel, dim3(B, H), dim3(64), 0, cur_stream(),
                     bf(out), partials.data_ptr<float>(), context_lens.data_ptr<int>(),
                     H, KVH, max_chunks, CHUNK_KEYS);
}

void attn_decode_paged(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                       torch::Tensor v_cache, torch::Tensor block_tables,
                       torch::Tensor context_lens, double scale,
                       torch::Tensor k_scale, torch::Tensor v_scale) {
  attn_decode_paged_impl(out, q, k_cache, v_cache, block_tables, context_lens, scale,
                         k_scale, v_scale, false, nullptr, nullptr, nullptr, nullptr, 0);
}

// Shared-prefix cascade: skip_chunks [B], tile_rows [n_tiles, 64],
// tile_nmembers [n_tiles], tile_chunks [n_tiles], all int32 on the GPU
// (engine.shared_prefix.build_shared_prefix_tiles). Zero tiles is the plain
// per-stream path.
void attn_decode_paged_shared(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                              torch::Tensor v_cache, torch::Tensor block_tables,
                              torch::Tensor context_lens, double scale,
                              torch::Tensor k_scale, torch::Tensor v_scale,
                              torch::Tensor skip_chunks, torch::Tensor tile_rows,
                              torch::Tensor tile_nmembers, torch::Tensor tile_chunks) {
  const int n_tiles = tile_nmembers.numel();
  auto ok = [](const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kInt;
  };
  TORCH_CHECK(ok(skip_chunks) && ok(tile_rows) && ok(tile_nmembers) && ok(tile_chunks),
              "attn_decode_paged_shared: metadata must be contiguous int32 on GPU");
  TORCH_CHECK(skip_chunks.numel() == q.size(0), "skip_chunks must be [B]");
  TORCH_CHECK(tile_rows.numel() == (int64_t)n_tiles * 64, "tile_rows must be [n_tiles, 64]");
  TORCH_CHECK(tile_chunks.numel() == n_tiles, "tile_chunks must be [n_tiles]");
  attn_decode_paged_impl(out, q, k_cache, v_cache, block_tables, context_lens, scale,
                         k_scale, v_scale, true, skip_chunks.data_ptr<int>(),
                         tile_rows.data_ptr<int>(), tile_nmembers.data_ptr<int>(),
                         tile_chunks.data_ptr<int>(), n_tiles);
}

void attn_prefill(torch::Tensor out, torch::Tensor q, torch::Tensor k, torch::Tensor v,
                  torch::Tensor grp_seq_start, torch::Tensor grp_qpos0,
                  torch::Tensor grp_seqlen, double scale) {
  CHECK_BF16_CONTIG(out); CHECK_BF16_ROWS(q); CHECK_BF16_ROWS(k); CHECK_BF16_ROWS(v);
  const int H = q.size(1), D = q.size(2), KVH = k.size(1);
  TORCH_CHECK(D == 128, "attn_prefill: head_dim must be 128");
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v must share the token stride");
  const int ngroups = grp_seq_start.size(0);
  TORCH_CHECK(grp_qpos0.size(0) == ngroups * 8, "grp_qpos0 must be [G*8]");
  hipLaunchKernelGGL(attn_prefill_kernel, dim3(ngroups, H), dim3(512), 0, cur_stream(),
                     bf(out), cbf(q), cbf(k), cbf(v),
                     grp_seq_start.data_ptr<int>(), grp_seqlen.data_ptr<int>(),
                     grp_qpos0.data_ptr<int>(), (float)scale, H, KVH,
                     (int)q.stride(0), (int)k.stride(0));
}

// The argument checks attn_prefill_paged and attn_prefill_paged_split share;
// `op` names the binding in the messages and `extra_meta` is the int32
// metadata only that binding takes.
struct PagedPrefillDims { int T, H, KVH, BS, n_seq, n_groups, cache_fp8; };

static PagedPrefillDims check_paged_prefill(
    const char* op, const torch::Tensor& out, const torch::Tensor& q,
    const torch::Tensor& k_cache, const torch::Tensor& v_cache,
    const torch::Tensor& block_tables, const torch::Tensor& cu_q, const torch::Tensor& q_start,
    const torch::Tensor& grp_seq, const torch::Tensor& grp_qpos0,
    const torch::Tensor& k_scale, const torch::Tensor& v_scale,
    std::initializer_list<torch::Tensor> extra_meta = {}) {
  CHECK_BF16_CONTIG(out); CHECK_BF16_ROWS(q); CHECK_KV_CACHE(k_cache); CHECK_KV_CACHE(v_cache);
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() &&
                  v_cache.scalar_type() == k_cache.scalar_type(),
              op, ": k_cache/v_cache must be [NB, KVH, BS, D] of one dtype");
  const int T = q.size(0), H = q.size(1), D = q.size(2);
  const int KVH = k_cache.size(1), BS = k_cache.size(2);
  TORCH_CHECK(D == 128 && k_cache.size(3) == 128, op, ": head_dim must be 128");
  TORCH_CHECK(KVH > 0 && H % KVH == 0, op, ": H must be a multiple of KVH");
  TORCH_CHECK(out.dim() == 3 && out.sizes() == q.sizes(), op, ": out must be [T, H, D]");
  TORCH_CHECK(q.stride(0) >= (int64_t)H * D && q.stride(0) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              op, ": q token stride must cover H*D and keep rows 16-byte aligned");
  auto ok = [](const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kInt;
  };
  TORCH_CHECK(ok(block_tables) && ok(cu_q) && ok(q_start) && ok(grp_seq) && ok(grp_qpos0) &&
                  std::all_of(extra_meta.begin(), extra_meta.end(), ok),
              op, ": metadata must be contiguous int32 on GPU");
  const int n_seq = q_start.numel();
  TORCH_CHECK(n_seq >= 1 && cu_q.numel() == n_seq + 1, "cu_q must be [n_seq + 1]");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == n_seq && block_tables.size(1) >= 1,
              "block_tables must be [n_seq, max_blocks]");
  const int n_groups = grp_seq.numel();
  TORCH_CHECK(grp_qpos0.numel() == (int64_t)n_groups * 8, "grp_qpos0 must be [G*8]");
  const int cache_fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn ? 1 : 0;
  if (cache_fp8) {
    TORCH_CHECK(k_scale.is_cuda() && v_scale.is_cuda() &&
                    k_scale.numel() == k_cache.size(0) * KVH * BS && k_scale.is_contiguous() &&
                    v_scale.is_contiguous() && k_scale.scalar_type() == at::kFloat &&
                    v_scale.scalar_type() == at::kFloat && v_scale.numel() == k_scale.numel(),
                "fp8 ", op, " requires [NB, KVH, BS] fp32 k_scale/v_scale");
  } else {
    TORCH_CHECK(k_scale.numel() == 0 && v_scale.numel() == 0,
                op, ": k_scale/v_scale go with fp8 caches only");
  }
  return {T, H, KVH, BS, n_seq, n_groups, cache_fp8};
}

// Paged (append / extend) prefill attention: new tokens packed at rows
// cu_q[s]..cu_q[s+1] attend causally to the q_start[s] keys already cached
// plus themselves, all read through block_tables[s] (one row per sequence).
// grp_seq [G] / grp_qpos0 [G*8] are the per-workgroup q-tiles of
// ops.build_paged_prefill, which also checks q_start + q_len against the
// table width on the host.
void attn_prefill_paged(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                        torch::Tensor v_cache, torch::Tensor block_tables, torch::Tensor cu_q,
                        torch::Tensor q_start, torch::Tensor grp_seq, torch::Tensor grp_qpos0,
                        double scale, torch::Tensor k_scale, torch::Tensor v_scale) {
  const PagedPrefillDims d = check_paged_prefill(
      "attn_prefill_paged", out, q, k_cache, v_cache, block_tables, cu_q, q_start, grp_seq,
      grp_qpos0, k_scale, v_scale);
  if (d.T == 0 || d.n_groups == 0) return;
  launch_attn_prefill_paged(
      bf(out), cbf(q), k_cache.data_ptr(), v_cache.data_ptr(),
      d.cache_fp8 ? k_scale.data_ptr<float>() : nullptr,
      d.cache_fp8 ? v_scale.data_ptr<float>() : nullptr,
      block_tables.data_ptr<int>(), cu_q.data_ptr<int>(), q_start.data_ptr<int>(),
      grp_seq.data_ptr<int>(), grp_qpos0.data_ptr<int>(), (float)scale, d.n_seq, d.T, d.H,
      d.KVH, (int)k_cache.size(0), d.BS, (int)block_tables.size(1), (int)q.stride(0),
      d.n_groups, d.cache_fp8, cur_stream());
}

// attn_prefill_paged with the keys of some sequences split across workgroups
// (ops.build_paged_prefill(key_splits=...)): grp_krange [G*2] is each
// workgroup's key range, grp_split [G] its split index (-1: the sequence is
// unsplit and the workgroup writes out directly), seq_nsplit / seq_ws_base
// [n_seq] the sequence's split count and first workspace slot. part_o
// [>= ws_rows, H, 128] and part_ml [>= ws_rows, H, 2] (fp32) take the
// partials, which a second kernel merges into out. ws_rows and max_splits are
// the plan's slot count and largest split count.
void attn_prefill_paged_split(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                              torch::Tensor v_cache, torch::Tensor block_tables,
                              torch::Tensor cu_q, torch::Tensor q_start, torch::Tensor grp_seq,
                              torch::Tensor grp_qpos0, torch::Tensor grp_krange,
                              torch::Tensor grp_split, torch::Tensor seq_nsplit,
                              torch::Tensor seq_ws_base, torch::Tensor part_o,
                              torch::Tensor part_ml, int64_t ws_rows, int64_t max_splits,
                              double scale, torch::Tensor k_scale, torch::Tensor v_scale) {
  const PagedPrefillDims d = check_paged_prefill(
      "attn_prefill_paged_split", out, q, k_cache, v_cache, block_tables, cu_q, q_start,
      grp_seq, grp_qpos0, k_scale, v_scale, {grp_krange, grp_split, seq_nsplit, seq_ws_base});
  TORCH_CHECK(grp_krange.numel() == (int64_t)d.n_groups * 2, "grp_krange must be [G*2]");
  TORCH_CHECK(grp_split.numel() == d.n_groups, "grp_split must be [G]");
  TORCH_CHECK(seq_nsplit.numel() == d.n_seq && seq_ws_base.numel() == d.n_seq,
              "seq_nsplit and seq_ws_base must be [n_seq]");
  TORCH_CHECK(max_splits >= 2 && max_splits <= 64,
              "attn_prefill_paged_split: max_splits must be 2..64");
  TORCH_CHECK(ws_rows >= 1 && ws_rows <= (int64_t)d.T * max_splits,
              "attn_prefill_paged_split: ws_rows must be 1..T*max_splits");
  auto ws_ok = [&](const torch::Tensor& t, int64_t last) {
    return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat && t.dim() == 3 &&
           t.size(0) >= ws_rows && t.size(1) == d.H && t.size(2) == last &&
           reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  TORCH_CHECK(ws_ok(part_o, 128) && ws_ok(part_ml, 2),
              "attn_prefill_paged_split: part_o / part_ml must be contiguous fp32 "
              "[>= ws_rows, H, 128] / [>= ws_rows, H, 2]");
  if (d.T == 0 || d.n_groups == 0) return;
  launch_attn_prefill_paged_split(
      bf(out), cbf(q), k_cache.data_ptr(), v_cache.data_ptr(),
      d.cache_fp8 ? k_scale.data_ptr<float>() : nullptr,
      d.cache_fp8 ? v_scale.data_ptr<float>() : nullptr,
      block_tables.data_ptr<int>(), cu_q.data_ptr<int>(), q_start.data_ptr<int>(),
      grp_seq.data_ptr<int>(), grp_qpos0.data_ptr<int>(), grp_krange.data_ptr<int>(),
      grp_split.data_ptr<int>(), seq_nsplit.data_ptr<int>(), seq_ws_base.data_ptr<int>(),
      part_o.data_ptr<float>(), part_ml.data_ptr<float>(), (int)ws_rows, (int)max_splits,
      (float)scale, d.n_seq, d.T, d.H, d.KVH, (int)k_cache.size(0), d.BS,
      (int)block_tables.size(1), (int)q.stride(0), d.n_groups, d.cache_fp8, cur_stream());
}

void sample(torch::Tensor tokens, torch::Tensor logprobs, torch::Tensor logits,
            torch::Tensor temperatures, torch::Tensor top_ps, torch::Tensor top_ks,
            torch::Tensor seeds, torch::Tensor steps, torch::Tensor mask,
            torch::Tensor dbg) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.scalar_type() == at::kFloat);
  const int B = logits.size(0), V = logits.size(1);
  const uint32_t* mptr = mask.numel() > 0
      ? reinterpret_cast<const uint32_t*>(mask.data_ptr<int>()) : nullptr;
  const size_t lds = 16 * 256 * (sizeof(float) + sizeof(unsigned int));  // per-wave histograms
  hipLaunchKernelGGL(sample_kernel, dim3(B), dim3(1024), lds, cur_stream(),
                     tokens.data_ptr<int64_t>(), logprobs.data_ptr<float>(),
                     logits.data_ptr<float>(), temperatures.data_ptr<float>(),
                     top_ps.data_ptr<float>(), top_ks.data_ptr<int>(),
                     seeds.data_ptr<int64_t>(), steps.data_ptr<int64_t>(), mptr, V,
                     dbg.numel() ? dbg.data_ptr<float>() : nullptr);
}

// Constrained sampling with the DFA state on the device: `tabs` [B, 6] holds
// per-stream device addresses of the constraint tables (the caller keeps the
// tables alive past the launch); `fsm_state` [B] is advanced in place.
void sample_fsm(torch::Tensor tokens, torch::Tensor logprobs, torch::Tensor logits,
                torch::Tensor temperatures, torch::Tensor top_ps, torch::Tensor top_ks,
                torch::Tensor seeds, torch::Tensor steps, torch::Tensor fsm_state,
                torch::Tensor tabs, int64_t eos_id) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.scalar_type() == at::kFloat &&
              logits.dim() == 2, "sample_fsm: logits must be contiguous fp32 [B, V] on GPU");
  const int B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(fsm_state.is_cuda() && fsm_state.device() == logits.device() &&
              fsm_state.is_contiguous() && fsm_state.scalar_type() == at::kInt &&
              fsm_state.dim() == 1 && fsm_state.size(0) == B,
              "sample_fsm: fsm_state must be contiguous int32 [B] on the logits device");
  TORCH_CHECK(tabs.is_cuda() && tabs.device() == logits.device() &&
              tabs.is_contiguous() && tabs.scalar_type() == at::kLong &&
              tabs.dim() == 2 && tabs.size(0) == B && tabs.size(1) == 6,
              "sample_fsm: tabs must be contiguous int64 [B, 6] on the logits device");
  TORCH_CHECK(tokens.is_cuda() && tokens.is_contiguous() && tokens.scalar_type() == at::kLong &&
              tokens.numel() == B, "sample_fsm: tokens must be contiguous int64 [B] on GPU");
  TORCH_CHECK(logprobs.is_cuda() && logprobs.is_contiguous() && logprobs.scalar_type() == at::kFloat &&
              logprobs.numel() == B, "sample_fsm: logprobs must be contiguous fp32 [B] on GPU");
  TORCH_CHECK(temperatures.numel() == B && top_ps.numel() == B && top_ks.numel() == B &&
              seeds.numel() == B && steps.numel() == B, "sample_fsm: per-row parameters must be [B]");
  TORCH_CHECK(eos_id >= -1 && eos_id < V, "sample_fsm: eos_id out of range");
  if (B == 0) return;
  const size_t lds = 16 * 256 * (sizeof(float) + sizeof(unsigned int));  // per-wave histograms
  hipLaunchKernelGGL(sample_fsm_kernel, dim3(B), dim3(1024), lds, cur_stream(),
                     tokens.data_ptr<int64_t>(), logprobs.data_ptr<float>(),
                     logits.data_ptr<float>(), temperatures.data_ptr<float>(),
                     top_ps.data_ptr<float>(), top_ks.data_ptr<int>(),
                     seeds.data_ptr<int64_t>(), steps.data_ptr<int64_t>(),
                     fsm_state.data_ptr<int>(), tabs.data_ptr<int64_t>(), (int)eos_id, V);
}

torch::Tensor mfma_selftest(torch::Tensor A, torch::Tensor B) {
  // D[32,32] = A[32,16] x B[16,32], verifying the fragment maps the attention
  // kernel assumes for v_mfma_f32_32x32x16_bf16.
  CHECK_BF16_CONTIG(A); CHECK_BF16_CONTIG(B);
  auto D = torch::empty({32, 32}, torch::dtype(torch::kFloat).device(A.device()));
  hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     D.data_ptr<float>(), cbf(A), cbf(B));
  return D;
}

extern "C" void launch_one_shot_allreduce(const void* const* srcs, void* const* dsts,
                                          int n_peers, long numel, int write_all,
                                          hipStream_t stream);

void one_shot_allreduce(std::vector<torch::Tensor> bufs) {
  // In-place sum across up to 8 same-shaped bf16 buffers (single-GPU
  // simulation of the one-shot xGMI all-reduce: every "peer" buffer ends
  // holding the fp32-accumulated sum). Multi-GPU wiring (IPC-mapped peer
  // pointers, write_all=0) is round-2 work — docs/ROADMAP.md item 1.
  TORCH_CHECK(!bufs.empty() && bufs.size() <= 8, "1..8 peer buffers");
  const auto numel = bufs[0].numel();
  TORCH_CHECK(numel % 8 == 0, "numel must be a multiple of 8 (16B vector path)");
  const void* srcs[8];
  void* dsts[8];
  for (size_t r = 0; r < bufs.size(); ++r) {
    CHECK_BF16_CONTIG(bufs[r]);
    TORCH_CHECK(bufs[r].numel() == numel, "peer buffers must match in size");
    srcs[r] = bufs[r].data_ptr();
    dsts[r] = bufs[r].data_ptr();
  }
  launch_one_shot_allreduce(srcs, dsts, (int)bufs.size(), (long)numel, /*write_all=*/1,
                            cur_stream());
}

// --- grouped MoE expert GEMMs (moe.hip) --------------------------------------
extern "C" void launch_moe_gateup(void* act, const void* x, const void* w, const float* scale,
                                  const int* sorted_ids, const int* pad_offsets,
                                  const void* zeros, int E, int IN, int K,
                                  hipStream_t stream);
extern "C" void launch_moe_down(void* y, const void* act, const void* w, const float* scale,
                                const int* pad_offsets, int E, int H, int IN,
                                hipStream_t stream);

// Expert weights [E, N, K]: bf16 with an empty `scale`, or e4m3 with fp32
// per-channel scales [E, N]. Returns the scale pointer (nullptr for bf16).
static const float* moe_weight_scale(const torch::Tensor& w, const torch::Tensor& scale) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.dim() == 3, "expert weights must be contiguous [E, N, K] on GPU");
  if (scale.numel() == 0) {
    TORCH_CHECK(w.scalar_type() == at::kBFloat16, "expert weights without scales must be bf16");
    return nullptr;
  }
  TORCH_CHECK(w.scalar_type() == at::kFloat8_e4m3fn, "expert weights with scales must be e4m3");
  TORCH_CHECK(scale.is_cuda() && scale.is_contiguous() && scale.scalar_type() == at::kFloat &&
              scale.dim() == 2 && scale.size(0) == w.size(0) && scale.size(1) == w.size(1),
              "expert scales must be contiguous fp32 [E, N] on GPU");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "e4m3 expert weights must be 16-byte aligned");
  return scale.data_ptr<float>();
}

// sorted_ids / pad_offsets: contiguous 1-D int32 on the GPU
static void check_moe_routing(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 1 && t.scalar_type() == at::kInt,
              name, " must be a contiguous 1-D int32 tensor on GPU");
}

// the kernels take raw pointers: every operand lives on the output's device
// (an empty tensor, the "no scales" placeholder, has no memory to be read)
static void check_moe_one_device(const torch::Tensor& out, std::initializer_list<torch::Tensor> ts) {
  for (const auto& t : ts)
    TORCH_CHECK(t.numel() == 0 || t.device() == out.device(),
                "grouped MoE operands must be on one device");
}

void moe_gateup(torch::Tensor act, torch::Tensor x, torch::Tensor w, torch::Tensor scale,
                torch::Tensor sorted_ids, torch::Tensor pad_offsets, torch::Tensor zeros) {
  CHECK_BF16_CONTIG(act); CHECK_BF16_CONTIG(x); CHECK_BF16_CONTIG(zeros);
  TORCH_CHECK(act.dim() == 2 && x.dim() == 2, "act and x must be 2-D");
  const float* sc = moe_weight_scale(w, scale);
  check_moe_routing(sorted_ids, "sorted_ids");
  check_moe_routing(pad_offsets, "pad_offsets");
  check_moe_one_device(act, {x, w, scale, zeros, sorted_ids, pad_offsets});
  const int E = w.size(0);
  const int IN = w.size(1) / 2;
  const int K = w.size(2);
  TORCH_CHECK(IN % 64 == 0 && K % 64 == 0, "IN % 64, K % 64 required");
  TORCH_CHECK(act.size(1) == IN && x.size(1) == K && zeros.numel() >= K);
  TORCH_CHECK(act.size(0) % 128 == 0, "sorted rows must be padded to 128");
  TORCH_CHECK(sorted_ids.numel() == act.size(0), "sorted_ids must have one entry per row of act");
  TORCH_CHECK(pad_offsets.numel() == E + 1);
  launch_moe_gateup(act.data_ptr(), x.data_ptr(), w.data_ptr(), sc,
                    sorted_ids.data_ptr<int>(), pad_offsets.data_ptr<int>(),
                    zeros.data_ptr(), E, IN, K, cur_stream());
}

void moe_down(torch::Tensor y, torch::Tensor act, torch::Tensor w, torch::Tensor scale,
              torch::Tensor pad_offsets) {
  CHECK_BF16_CONTIG(y); CHECK_BF16_CONTIG(act);
  TORCH_CHECK(y.dim() == 2 && act.dim() == 2, "y and act must be 2-D");
  const float* sc = moe_weight_scale(w, scale);
  check_moe_routing(pad_offsets, "pad_offsets");
  check_moe_one_device(y, {act, w, scale, pad_offsets});
  const int E = w.size(0);
  const int H = w.size(1);
  const int IN = w.size(2);
  TORCH_CHECK(H % 64 == 0 && IN % 64 == 0, "H % 64, IN % 64 required");
  TORCH_CHECK(y.size(1) == H && act.size(1) == IN);
  TORCH_CHECK(y.size(0) == act.size(0), "y and act must have the same sorted rows");
  TORCH_CHECK(y.size(0) % 128 == 0, "sorted rows must be padded to 128");
  TORCH_CHECK(pad_offsets.numel() == E + 1);
  launch_moe_down(y.data_ptr(), act.data_ptr(), w.data_ptr(), sc,
                  pad_offsets.data_ptr<int>(), E, H, IN, cur_stream());
}

// --- batched Levenshtein (levenshtein.hip) -----------------------------------
extern "C" void launch_levenshtein(int* out, const unsigned char* chars, const int* lens,
                                   const int* pi, const int* pj, long n_pairs,
                                   hipStream_t stream);

torch::Tensor levenshtein_pairs(torch::Tensor chars, torch::Tensor lens,
                                torch::Tensor pair_i, torch::Tensor pair_j) {
  TORCH_CHECK(chars.is_cuda() && chars.scalar_type() == at::kByte && chars.size(1) == 64 &&
              chars.is_contiguous(), "chars must be contiguous uint8 [N, 64] on GPU");
  TORCH_CHECK(lens.scalar_type() == at::kInt && pair_i.scalar_type() == at::kInt &&
              pair_j.scalar_type() == at::kInt);
  const long P = pair_i.numel();
  auto out = torch::empty({P}, torch::dtype(torch::kInt).device(chars.device()));
  launch_levenshtein(out.data_ptr<int>(),
                     chars.data_ptr<unsigned char>(), lens.data_ptr<int>(),
                     pair_i.data_ptr<int>(), pair_j.data_ptr<int>(), P, cur_stream());
  return out;
}

// --- hipIpc one-shot all-reduce (allreduce.hip) ------------------------------
extern "C" void* ipc_ar_create(int rank, int world, size_t max_bytes, unsigned char* handles_out);
extern "C" int ipc_ar_connect(void* ctx, const unsigned char* all_handles);
extern "C" int ipc_ar_run(void* ctx, const void* inp, void* out, long numel, hipStream_t stream);
extern "C" void ipc_ar_destroy(void* ctx);

std::pair<int64_t, py::bytes> ipc_allreduce_create(int rank, int world, int64_t max_bytes) {
  unsigned char handles[128];
  void* ctx = ipc_ar_create(rank, world, (size_t)max_bytes, handles);
  TORCH_CHECK(ctx != nullptr, "ipc_ar_create failed (see stderr)");
  return {reinterpret_cast<int64_t>(ctx), py::bytes(reinterpret_cast<char*>(handles), 128)};
}

void ipc_allreduce_connect(int64_t ctx, py::bytes all_handles) {
  std::string h = all_handles;
  TORCH_CHECK(h.size() % 128 == 0, "handle blob must be world*128 bytes");
  int rc = ipc_ar_connect(reinterpret_cast<void*>(ctx),
                          reinterpret_cast<const unsigned char*>(h.data()));
  TORCH_CHECK(rc == 0, "ipc_ar_connect failed (see stderr)");
}

void ipc_allreduce_run(int64_t ctx, torch::Tensor inp, torch::Tensor out) {
  CHECK_BF16_CONTIG(inp);
  CHECK_BF16_CONTIG(out);
  TORCH_CHECK(inp.numel() == out.numel(), "in/out size mismatch");
  int rc = ipc_ar_run(reinterpret_cast<void*>(ctx), inp.data_ptr(), out.data_ptr(),
                      (long)inp.numel(), cur_stream());
  TORCH_CHECK(rc == 0, "ipc_ar_run failed rc=", rc);
}

void ipc_allreduce_destroy(int64_t ctx) {
  ipc_ar_destroy(reinterpret_cast<void*>(ctx));
}

// --- weight-only fp8 GEMM (linear_fp8w.hip) ------------------------------------
extern "C" void linear_fp8w_plan(int M, int N, int K, int n_cus, int* mt, int* splitk);
extern "C" void launch_linear_fp8w(void* out, float* slabs, const void* x, const void* q,
                                   const float* scale, const void* bias, int M, int N, int K,
                                   long x_stride, int mt, int splitk, hipStream_t stream);
extern "C" void launch_dequant_fp8w(void* w, const void* q, const float* scale, long numel,
                                    int K, hipStream_t stream);
extern "C" void linear_fp8w_batched_plan(int E, int M, int N, int K, int n_cus, int* mt,
                                         int* splitk);
extern "C" void launch_linear_fp8w_batched(void* out, float* slabs, const void* x,
                                           const void* q, const float* scale, int E, int M,
                                           int N, int K, long x_stride, long x_bstride, int mt,
                                           int splitk, hipStream_t stream);

#define CHECK_FP8W(q, scale)                                                             \
  TORCH_CHECK((q).is_cuda() && (q).is_contiguous() && (q).dim() == 2 &&                  \
              (q).scalar_type() == at::kFloat8_e4m3fn, "q must be contiguous e4m3 [N, K] on GPU"); \
  TORCH_CHECK((scale).is_cuda() && (scale).is_contiguous() &&                            \
              (scale).scalar_type() == at::kFloat && (scale).numel() == (q).size(0),     \
              "scale must be contiguous fp32 [N] on GPU")

// out[M, N] = bf16((x @ q^T) * scale + bias); bias: bf16 [N] or an empty tensor.
// Takes 1 <= M <= 256, K % 64 == 0, N % 16 == 0, x with unit inner stride and
// a 16-byte-aligned row stride >= K (ops.linear_fp8w routes everything else
// through dequant_fp8w).
void linear_fp8w(torch::Tensor out, torch::Tensor x, torch::Tensor q, torch::Tensor scale,
                 torch::Tensor bias) {
  CHECK_FP8W(q, scale);
  const int64_t M = x.size(0), K = x.size(1), N = q.size(0);
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 &&
              x.stride(1) == 1 && x.stride(0) >= K && x.stride(0) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "linear_fp8w: x must be a bf16 [M, K] row view with 16-byte-aligned rows");
  TORCH_CHECK(q.size(1) == K, "linear_fp8w: x and q disagree on K");
  TORCH_CHECK(M >= 1 && M <= 256 && K % 64 == 0 && N % 16 == 0,
              "linear_fp8w: needs 1 <= M <= 256, K % 64 == 0, N % 16 == 0; got M=", M,
              " N=", N, " K=", K);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 && out.is_contiguous() &&
              out.dim() == 2 && out.size(0) == M && out.size(1) == N,
              "linear_fp8w: out must be contiguous bf16 [M, N]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(scale.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "linear_fp8w: q/scale must be 16-byte aligned, out 8-byte aligned");
  const void* bptr = nullptr;
  if (bias.numel() > 0) {
    TORCH_CHECK(bias.is_cuda() && bias.is_contiguous() && bias.scalar_type() == at::kBFloat16 &&
                bias.numel() == N && reinterpret_cast<uintptr_t>(bias.data_ptr()) % 8 == 0,
                "linear_fp8w: bias must be contiguous bf16 [N]");
    bptr = bias.data_ptr();
  }
  const int n_cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  int mt = 1, splitk = 1;
  linear_fp8w_plan((int)M, (int)N, (int)K, n_cus, &mt, &splitk);
  float* slabs = nullptr;
  torch::Tensor ws;
  if (splitk > 1) {
    ws = torch::empty({(int64_t)splitk * M * N}, torch::dtype(torch::kFloat).device(x.device()));
    slabs = ws.data_ptr<float>();
  }
  launch_linear_fp8w(out.data_ptr(), slabs, x.data_ptr(), q.data_ptr(), scale.data_ptr<float>(),
                     bptr, (int)M, (int)N, (int)K, (long)x.stride(0), mt, splitk, cur_stream());
}

// out[e] = bf16((x_e @ q[e]^T) * scale[e]) for the E experts of q [E, N, K]; x is
// [M, K] (shared by all experts) or [E, M, K], unit inner stride, row and batch
// strides multiples of 8 elements. Same shape limits as linear_fp8w.
void linear_fp8w_batched(torch::Tensor out, torch::Tensor x, torch::Tensor q,
                         torch::Tensor scale) {
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() && q.dim() == 3 &&
              q.scalar_type() == at::kFloat8_e4m3fn,
              "linear_fp8w_batched: q must be contiguous e4m3 [E, N, K] on GPU");
  const int64_t E = q.size(0), N = q.size(1), K = q.size(2);
  TORCH_CHECK(scale.is_cuda() && scale.is_contiguous() && scale.scalar_type() == at::kFloat &&
              scale.dim() == 2 && scale.size(0) == E && scale.size(1) == N,
              "linear_fp8w_batched: scale must be contiguous fp32 [E, N] on GPU");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && (x.dim() == 2 || x.dim() == 3),
              "linear_fp8w_batched: x must be bf16 [M, K] or [E, M, K] on GPU");
  const bool shared = x.dim() == 2;
  const int64_t M = x.size(shared ? 0 : 1);
  const int64_t x_stride = x.stride(shared ? 0 : 1);
  const int64_t x_bstride = shared ? 0 : x.stride(0);
  TORCH_CHECK(x.size(-1) == K && (shared || x.size(0) == E),
              "linear_fp8w_batched: x and q disagree on E or K");
  TORCH_CHECK(E >= 1 && E <= 1024 && M >= 1 && M <= 256 && K % 64 == 0 && N % 16 == 0,
              "linear_fp8w_batched: needs 1 <= E <= 1024, 1 <= M <= 256, K % 64 == 0, "
              "N % 16 == 0; got E=", E, " M=", M, " N=", N, " K=", K);
  TORCH_CHECK(x.stride(-1) == 1 && x_stride >= K && x_stride % 8 == 0 && x_bstride % 8 == 0 &&
              reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "linear_fp8w_batched: x needs unit inner stride and 16-byte-aligned rows and experts");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 && out.is_contiguous() &&
              out.dim() == 3 && out.size(0) == E && out.size(1) == M && out.size(2) == N,
              "linear_fp8w_batched: out must be contiguous bf16 [E, M, N]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(scale.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "linear_fp8w_batched: q/scale must be 16-byte aligned, out 8-byte aligned");
  const int n_cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  int mt = 1, splitk = 1;
  linear_fp8w_batched_plan((int)E, (int)M, (int)N, (int)K, n_cus, &mt, &splitk);
  float* slabs = nullptr;
  torch::Tensor ws;
  if (splitk > 1) {
    ws = torch::empty({E * splitk * M * N}, torch::dtype(torch::kFloat).device(x.device()));
    slabs = ws.data_ptr<float>();
  }
  launch_linear_fp8w_batched(out.data_ptr(), slabs, x.data_ptr(), q.data_ptr(),
                             scale.data_ptr<float>(), (int)E, (int)M, (int)N, (int)K,
                             (long)x_stride, (long)x_bstride, mt, splitk, cur_stream());
}

// w[N, K] = bf16(fp32(q) * scale[n]) into the first N*K elements of `w` (a
// reusable bf16 scratch); K % 16 == 0.
void dequant_fp8w(torch::Tensor w, torch::Tensor q, torch::Tensor scale) {
  CHECK_FP8W(q, scale);
  CHECK_BF16_CONTIG(w);
  TORCH_CHECK(w.numel() >= q.numel(), "dequant_fp8w: scratch smaller than the weight");
  TORCH_CHECK(q.size(1) % 16 == 0, "dequant_fp8w: K must be a multiple of 16");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "dequant_fp8w: q and w must be 16-byte aligned");
  if (q.numel() == 0) return;
  launch_dequant_fp8w(w.data_ptr(), q.data_ptr(), scale.data_ptr<float>(), (long)q.numel(),
                      (int)q.size(1), cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("linear_fp8w", &linear_fp8w);
  m.def("linear_fp8w_batched", &linear_fp8w_batched);
  m.def("dequant_fp8w", &dequant_fp8w);
  m.def("levenshtein_pairs", &levenshtein_pairs);
  m.def("moe_gateup", &moe_gateup);
  m.def("moe_down", &moe_down);
  m.def("ipc_allreduce_create", &ipc_allreduce_create);
  m.def("ipc_allreduce_connect", &ipc_allreduce_connect);
  m.def("ipc_allreduce_run", &ipc_allreduce_run);
  m.def("ipc_allreduce_destroy", &ipc_allreduce_destroy);
  m.def("rmsnorm", &rmsnorm);
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm);
  m.def("silu_mul", &silu_mul);
  m.def("rope_inplace", &rope_inplace);
  m.def("store_kv", &store_kv);
  m.def("rope_store_kv", &rope_store_kv);
  m.def("copy_kv_blocks", &copy_kv_blocks);
  m.def("attn_decode_paged", &attn_decode_paged);
  m.def("attn_decode_paged_shared", &attn_decode_paged_shared);
  m.def("attn_prefill", &attn_prefill);
  m.def("attn_prefill_paged", &attn_prefill_paged);
  m.def("attn_prefill_paged_split", &attn_prefill_paged_split);
  m.def("sample", &sample);
  m.def("sample_fsm", &sample_fsm);
  m.def("mfma_selftest", &mfma_selftest);
  m.def("one_shot_allreduce", &one_shot_allreduce);
}
