// PyTorch bindings for the kllms_amd gfx950 kernels (kllms_amd._C): the only
// host code that hands raw pointers to the kernels. A binding checks its
// arguments with the shared check functions below, returns when there are no
// rows, and calls the launcher that launch.h declares; grids, blocks and LDS
// sizes belong to the kernel TUs. No check reads device memory or synchronises
// (bindings run inside hipGraph capture); index VALUES stay the caller's
// contract, as launch.h says.

#include <algorithm>
#include <functional>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "launch.h"

using torch::Tensor;

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

static bf16_t* bf(const Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }
static const bf16_t* cbf(const Tensor& t) { return reinterpret_cast<const bf16_t*>(t.data_ptr()); }

// --- the check vocabulary ------------------------------------------------------

static bool aligned(const Tensor& t, uintptr_t bytes) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0;
}

// a dense (contiguous) GPU tensor of one dtype ...
static void check_dense(const char* op, const char* name, const Tensor& t, at::ScalarType dtype) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == dtype,
              op, ": ", name, " must be a contiguous ", dtype, " tensor on GPU");
}

// ... of exactly this shape
static void check_dense(const char* op, const char* name, const Tensor& t, at::ScalarType dtype,
                        at::IntArrayRef sizes) {
  check_dense(op, name, t, dtype);
  TORCH_CHECK(t.sizes() == sizes, op, ": ", name, " must be ", sizes, ", got ", t.sizes());
}

// ... of n elements: index tensors (int32 / int64) and per-row parameters
static void check_vec(const char* op, const char* name, const Tensor& t, at::ScalarType dtype,
                      int64_t n) {
  check_dense(op, name, t, dtype);
  TORCH_CHECK(t.numel() == n, op, ": ", name, " must have ", n, " elements, got ", t.numel());
}

// bf16 [T, H, D] activation view: head/dim dims packed, token stride free (so
// the fused-QKV splits need no .contiguous() copies), every row 16-byte aligned
static void check_rows(const char* op, const char* name, const Tensor& t) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.dim() == 3 &&
                  t.stride(2) == 1 && t.stride(1) == t.size(2) &&
                  t.stride(0) >= t.size(1) * t.size(2),
              op, ": ", name, " must be a bf16 [T, H, D] row view on GPU");
  TORCH_CHECK(t.size(2) % 8 == 0 && t.stride(0) % 8 == 0 && aligned(t, 16),
              op, ": ", name, " needs D % 8 == 0 and 16-byte-aligned rows");
}

// paged cache pair [NB, KVH, BS, D], both bf16 or both e4m3
struct CacheDims { int64_t NB, KVH, BS, D; int fp8; };

static CacheDims check_cache_pair(const char* op, const Tensor& k_cache, const Tensor& v_cache) {
  const auto dt = k_cache.scalar_type();
  TORCH_CHECK(dt == at::kBFloat16 || dt == at::kFloat8_e4m3fn,
              op, ": the KV cache must be bf16 or fp8-e4m3");
  check_dense(op, "k_cache", k_cache, dt);
  check_dense(op, "v_cache", v_cache, dt);
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes(),
              op, ": k_cache/v_cache must be [NB, KVH, BS, D] of one dtype");
  return {k_cache.size(0), k_cache.size(1), k_cache.size(2), k_cache.size(3),
          dt == at::kFloat8_e4m3fn ? 1 : 0};
}

// fp8 caches go with fp32 [NB, KVH, BS] per-row scales, bf16 caches with empty
// placeholders; returns the two pointers (null for bf16)
static std::pair<float*, float*> kv_scales(const char* op, const Tensor& k_cache,
                                           const Tensor& k_scale, const Tensor& v_scale) {
  if (k_cache.scalar_type() != at::kFloat8_e4m3fn) {
    TORCH_CHECK(k_scale.numel() == 0 && v_scale.numel() == 0,
                op, ": k_scale/v_scale go with fp8 caches only");
    return {nullptr, nullptr};
  }
  const int64_t n = k_cache.size(0) * k_cache.size(1) * k_cache.size(2);
  TORCH_CHECK(k_scale.is_cuda() && v_scale.is_cuda() && k_scale.is_contiguous() &&
                  v_scale.is_contiguous() && k_scale.scalar_type() == at::kFloat &&
                  v_scale.scalar_type() == at::kFloat && k_scale.numel() == n &&
                  v_scale.numel() == n,
              "fp8 ", op, " requires [NB, KVH, BS] fp32 k_scale/v_scale");
  return {k_scale.data_ptr<float>(), v_scale.data_ptr<float>()};
}

// the kernels take raw pointers: every operand lives on out's device (an empty
// tensor, the "no scales" placeholder, has no memory to be read)
static void check_one_device(const char* op, const Tensor& out,
                             std::initializer_list<std::reference_wrapper<const Tensor>> ts) {
  for (const Tensor& t : ts)
    TORCH_CHECK(t.numel() == 0 || t.device() == out.device(),
                op, ": all operands must be on one device");
}

// --- elementwise (elementwise.hip) ---------------------------------------------

// The checks rmsnorm and fused_add_rmsnorm share: out / x / (residual) dense
// bf16 of one shape [..., n], weight [n]. Returns {rows, n}.
static std::pair<int, int> check_rmsnorm(const char* op, const Tensor& out, const Tensor& x,
                                         const Tensor* residual, const Tensor& weight) {
  check_dense(op, "out", out, at::kBFloat16);
  check_dense(op, "x", x, at::kBFloat16);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0 && x.size(-1) % 8 == 0,
              op, ": hidden size must be a multiple of 8");
  TORCH_CHECK(out.sizes() == x.sizes(), op, ": out and x disagree on shape");
  const int64_t n = x.size(-1), rows = x.numel() / n;
  check_vec(op, "weight", weight, at::kBFloat16, n);
  TORCH_CHECK(aligned(out, 16) && aligned(x, 16) && aligned(weight, 16),
              op, ": operands must be 16-byte aligned");
  TORCH_CHECK(rows <= INT32_MAX, op, ": too many rows");
  check_one_device(op, out, {x, weight});
  if (residual) {
    check_dense(op, "residual", *residual, at::kBFloat16, x.sizes());
    TORCH_CHECK(aligned(*residual, 16) && residual->device() == out.device(),
                op, ": residual must be 16-byte aligned on out's device");
  }
  return {(int)rows, (int)n};
}

void rmsnorm(Tensor out, Tensor in, Tensor weight, double eps) {
  const auto [rows, n] = check_rmsnorm("rmsnorm", out, in, nullptr, weight);
  if (rows == 0) return;
  launch_rmsnorm(bf(out), cbf(in), cbf(weight), rows, n, (float)eps, cur_stream());
}

void fused_add_rmsnorm(Tensor out, Tensor x, Tensor residual, Tensor weight, double eps) {
  const auto [rows, n] = check_rmsnorm("fused_add_rmsnorm", out, x, &residual, weight);
  if (rows == 0) return;
  launch_fused_add_rmsnorm(bf(out), cbf(x), bf(residual), cbf(weight), rows, n, (float)eps,
                           cur_stream());
}

void silu_mul(Tensor out, Tensor gate, Tensor up) {
  const char* op = "silu_mul";
  auto row_view = [](const Tensor& t) {
    return t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.dim() == 2 && t.stride(1) == 1;
  };
  TORCH_CHECK(row_view(gate) && row_view(up), op, ": gate/up must be bf16 [T, I] row views on GPU");
  TORCH_CHECK(up.sizes() == gate.sizes() && up.stride(0) == gate.stride(0),
              op, ": gate and up disagree on shape or row stride");
  check_dense(op, "out", out, at::kBFloat16, gate.sizes());
  const int64_t ncols = gate.size(1), stride = gate.stride(0);
  TORCH_CHECK(ncols % 8 == 0 && stride % 8 == 0 && stride >= ncols && aligned(out, 16) &&
                  aligned(gate, 16) && aligned(up, 16),
              op, ": needs I % 8 == 0 and 16-byte-aligned rows");
  check_one_device(op, out, {gate, up});
  if (gate.numel() == 0) return;
  launch_silu_mul(bf(out), cbf(gate), cbf(up), gate.size(0), ncols, stride, cur_stream());
}

// The checks of everything rope_inplace, store_kv and rope_store_kv take; q,
// positions and cos_sin are null for store_kv; v, the caches, slot_mapping and
// the scales are null for rope_inplace. Returns the dimensions and scale pointers.
struct RopeStore { int T, H, KVH, D, BS, fp8; float *k_scale, *v_scale; };

static RopeStore check_rope_store(const char* op, const Tensor* q, const Tensor& k, const Tensor* v,
                                  const Tensor* positions, const Tensor* cos_sin,
                                  const Tensor* k_cache, const Tensor* v_cache,
                                  const Tensor* slot_mapping, const Tensor* k_scale,
                                  const Tensor* v_scale) {
  check_rows(op, "k", k);
  RopeStore r{(int)k.size(0), 0, (int)k.size(1), (int)k.size(2), 0, 0, nullptr, nullptr};
  if (q) {
    check_rows(op, "q", *q);
    TORCH_CHECK(q->size(0) == r.T && q->size(2) == r.D, op, ": q/k disagree on T or D");
    r.H = q->size(1);
    check_vec(op, "positions", *positions, at::kLong, r.T);
    check_dense(op, "cos_sin", *cos_sin, at::kFloat);
    TORCH_CHECK(cos_sin->dim() >= 1 && cos_sin->size(-1) == r.D, op, ": cos_sin must be [max_pos, D]");
    TORCH_CHECK(r.D >= 2 && r.D / 2 <= 1024, op, ": head_dim must be 2..2048");
    check_one_device(op, k, {*q, *positions, *cos_sin});
  }
  if (v) {
    check_rows(op, "v", *v);
    TORCH_CHECK(v->sizes() == k.sizes(), op, ": k/v disagree on T, KVH or D");
    const CacheDims c = check_cache_pair(op, *k_cache, *v_cache);
    TORCH_CHECK(c.KVH == r.KVH && c.D == r.D && c.BS > 0,
                op, ": caches must be [NB, KVH, BS, D] with k's KVH and D");
    check_vec(op, "slot_mapping", *slot_mapping, at::kLong, r.T);
    std::tie(r.k_scale, r.v_scale) = kv_scales(op, *k_cache, *k_scale, *v_scale);
    check_one_device(op, k, {*v, *k_cache, *v_cache, *slot_mapping, *k_scale, *v_scale});
    r.BS = c.BS;
    r.fp8 = c.fp8;
  }
  return r;
}

void rope_inplace(Tensor q, Tensor k, Tensor positions, Tensor cos_sin) {
  const RopeStore r = check_rope_store("rope_inplace", &q, k, nullptr, &positions, &cos_sin,
                                       nullptr, nullptr, nullptr, nullptr, nullptr);
  if (r.T == 0) return;
  launch_rope(bf(q), bf(k), positions.data_ptr<int64_t>(), cos_sin.data_ptr<float>(), r.T, r.H,
              r.KVH, r.D, (int)q.stride(0), (int)k.stride(0), cur_stream());
}

void store_kv(Tensor k, Tensor v, Tensor k_cache, Tensor v_cache, Tensor slot_mapping,
              Tensor k_scale, Tensor v_scale) {
  const RopeStore r = check_rope_store("store_kv", nullptr, k, &v, nullptr, nullptr, &k_cache,
                                       &v_cache, &slot_mapping, &k_scale, &v_scale);
  TORCH_CHECK(k.stride(0) == v.stride(0), "store_kv: k/v must share the token stride");
  if (r.T == 0) return;
  launch_store_kv(cbf(k), cbf(v), k_cache.data_ptr(), v_cache.data_ptr(), r.k_scale, r.v_scale,
                  slot_mapping.data_ptr<int64_t>(), r.T, r.KVH, r.D, r.BS, (int)k.stride(0),
                  r.fp8, cur_stream());
}

// rope_inplace + store_kv in one launch: q/k rotated in place, the rotated k
// and the untouched v scattered to the paged caches at slot_mapping. Same
// views and the same bits as the two separate ops.
void rope_store_kv(Tensor q, Tensor k, Tensor v, Tensor positions, Tensor cos_sin, Tensor k_cache,
                   Tensor v_cache, Tensor slot_mapping, Tensor k_scale, Tensor v_scale) {
  const RopeStore r = check_rope_store("rope_store_kv", &q, k, &v, &positions, &cos_sin, &k_cache,
                                       &v_cache, &slot_mapping, &k_scale, &v_scale);
  if (r.T == 0) return;
  launch_rope_store_kv(bf(q), bf(k), cbf(v), k_cache.data_ptr(), v_cache.data_ptr(), r.k_scale,
                       r.v_scale, positions.data_ptr<int64_t>(), cos_sin.data_ptr<float>(),
                       slot_mapping.data_ptr<int64_t>(), r.T, r.H, r.KVH, r.D, r.BS,
                       (int)q.stride(0), (int)k.stride(0), (int)v.stride(0), r.fp8, cur_stream());
}

// Copy blocks src[i] -> dst[i] of the two [L, NB, ...] arrays `a` and `b` (K
// and V, or the two fp8 scale arrays) for every layer in one launch
// (kv_copy.hip). src/dst: int32 [n] on the GPU, validated by the caller
// (in range, no block both a source and a destination).
void copy_kv_blocks(Tensor a, Tensor b, Tensor src, Tensor dst) {
  const char* op = "copy_kv_blocks";
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.is_contiguous() && b.is_contiguous() &&
              a.dim() >= 2 && a.sizes() == b.sizes() && a.scalar_type() == b.scalar_type(),
              op, ": a/b must be contiguous [L, NB, ...] GPU arrays of one shape and dtype");
  const int64_t n = src.numel(), L = a.size(0), NB = a.size(1);
  check_dense(op, "src", src, at::kInt, {n});
  check_dense(op, "dst", dst, at::kInt, {n});
  TORCH_CHECK(src.device() == a.device() && dst.device() == a.device(),
              op, ": src/dst must be on the arrays' device");
  if (n == 0 || L == 0 || NB == 0) return;
  TORCH_CHECK(n <= INT32_MAX / 2 / L, op, ": too many pairs");
  const int64_t block_bytes = a.stride(1) * (int64_t)a.element_size();
  const int64_t layer_stride = a.stride(0) * (int64_t)a.element_size();
  const uintptr_t bits = reinterpret_cast<uintptr_t>(a.data_ptr()) |
                         reinterpret_cast<uintptr_t>(b.data_ptr()) |
                         (uintptr_t)block_bytes | (uintptr_t)layer_stride;
  const int vec = bits % 16 == 0 ? 16 : (bits % 4 == 0 ? 4 : 1);
  launch_copy_kv_blocks(a.data_ptr(), b.data_ptr(), src.data_ptr<int>(), dst.data_ptr<int>(),
                        (int)n, (int)L, layer_stride, block_bytes, vec, cur_stream());
}

// --- decode attention (attn_decode.hip, attn_decode_shared.hip) ----------------

// Shared-prefix cascade metadata: skip_chunks [B], tile_rows [n_tiles, 64],
// tile_nmembers [n_tiles], tile_chunks [n_tiles], all int32 on the GPU
// (engine.shared_prefix.build_shared_prefix_tiles).
struct SharedTiles { const Tensor &skip_chunks, &tile_rows, &tile_nmembers, &tile_chunks; };

// Body of the two decode-attention bindings. Without `tiles` (or with zero
// tiles) this is exactly the per-stream split-K path; with them the
// shared-prefix kernel first writes the partials of each group's leading
// chunks and the per-stream kernel skips them. The reduce is the same.
static void attn_decode_paged_impl(const char* op, Tensor& out, Tensor& q, Tensor& k_cache,
                                   Tensor& v_cache, Tensor& block_tables, Tensor& context_lens,
                                   double scale, Tensor& k_scale, Tensor& v_scale,
                                   const SharedTiles* tiles) {
  check_rows(op, "q", q);
  check_dense(op, "out", out, at::kBFloat16, q.sizes());
  const CacheDims c = check_cache_pair(op, k_cache, v_cache);
  const int B = q.size(0), H = q.size(1), KVH = c.KVH, BS = c.BS;
  TORCH_CHECK(q.size(2) == 128 && c.D == 128, op, ": head_dim must be 128");
  TORCH_CHECK(KVH > 0 && H % KVH == 0, op, ": H must be a multiple of KVH");
  const int gqa = H / KVH;
  TORCH_CHECK(gqa == 1 || gqa == 2 || gqa == 4 || gqa == 8, op, ": GQA group must be 1, 2, 4 or 8");
  check_dense(op, "block_tables", block_tables, at::kInt);
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == B,
              op, ": block_tables must be [B, max_blocks]");
  check_vec(op, "context_lens", context_lens, at::kInt, B);
  const auto [ks, vs] = kv_scales(op, k_cache, k_scale, v_scale);
  check_one_device(op, out, {q, k_cache, v_cache, block_tables, context_lens, k_scale, v_scale});
  int n_tiles = 0;
  if (tiles) {
    n_tiles = tiles->tile_nmembers.numel();
    check_vec(op, "skip_chunks", tiles->skip_chunks, at::kInt, B);
    check_vec(op, "tile_rows", tiles->tile_rows, at::kInt, (int64_t)n_tiles * 64);
    check_vec(op, "tile_nmembers", tiles->tile_nmembers, at::kInt, n_tiles);
    check_vec(op, "tile_chunks", tiles->tile_chunks, at::kInt, n_tiles);
    check_one_device(op, out, {tiles->skip_chunks, tiles->tile_rows, tiles->tile_nmembers,
                               tiles->tile_chunks});
  }
  if (B == 0) return;
  const int max_blocks = block_tables.size(1);
  // split-K granule: fixed 256 keys measured best across B=40..240 and
  // ctx 576..2048 (adaptive coarser chunks trade combine traffic for lost
  // block-level parallelism and net 0..-5%; chunk size stays a runtime arg)
  const int CHUNK_KEYS = ATTN_DECODE_TKV;  // 256
  const int max_chunks = std::max(1, (max_blocks * BS + CHUNK_KEYS - 1) / CHUNK_KEYS);
  auto partials = torch::empty({attn_decode_partials_numel(B, H, max_chunks)},
                               torch::dtype(torch::kFloat).device(q.device()));
  if (n_tiles > 0) {
    launch_attn_decode_shared(
        partials.data_ptr<float>(), cbf(q), k_cache.data_ptr(), v_cache.data_ptr(), ks, vs,
        block_tables.data_ptr<int>(), tiles->tile_rows.data_ptr<int>(),
        tiles->tile_nmembers.data_ptr<int>(), tiles->tile_chunks.data_ptr<int>(), (float)scale,
        B, H, KVH, (int)c.NB, BS, max_blocks, max_chunks, (int)q.stride(0), n_tiles, c.fp8,
        cur_stream());
  }
  launch_attn_decode_partial(
      partials.data_ptr<float>(), cbf(q), k_cache.data_ptr(), v_cache.data_ptr(), ks, vs,
      block_tables.data_ptr<int>(), context_lens.data_ptr<int>(),
      n_tiles > 0 ? tiles->skip_chunks.data_ptr<int>() : nullptr, (float)scale, H, KVH, BS,
      max_blocks, max_chunks, (int)q.stride(0), CHUNK_KEYS, B, c.fp8, cur_stream());
  launch_attn_decode_reduce(bf(out), partials.data_ptr<float>(), context_lens.data_ptr<int>(), B,
                            H, KVH, max_chunks, CHUNK_KEYS, cur_stream());
}

void attn_decode_paged(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables,
                       Tensor context_lens, double scale, Tensor k_scale, Tensor v_scale) {
  attn_decode_paged_impl("attn_decode_paged", out, q, k_cache, v_cache, block_tables,
                         context_lens, scale, k_scale, v_scale, nullptr);
}

void attn_decode_paged_shared(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache,
                              Tensor block_tables, Tensor context_lens, double scale,
                              Tensor k_scale, Tensor v_scale, Tensor skip_chunks,
                              Tensor tile_rows, Tensor tile_nmembers, Tensor tile_chunks) {
  const SharedTiles tiles{skip_chunks, tile_rows, tile_nmembers, tile_chunks};
  attn_decode_paged_impl("attn_decode_paged_shared", out, q, k_cache, v_cache, block_tables,
                         context_lens, scale, k_scale, v_scale, &tiles);
}

// --- prefill attention (attn_prefill.hip, attn_prefill_paged.hip) --------------

void attn_prefill(Tensor out, Tensor q, Tensor k, Tensor v, Tensor grp_seq_start,
                  Tensor grp_qpos0, Tensor grp_seqlen, double scale) {
  const char* op = "attn_prefill";
  check_rows(op, "q", q); check_rows(op, "k", k); check_rows(op, "v", v);
  check_dense(op, "out", out, at::kBFloat16, q.sizes());
  const int64_t T = q.size(0), H = q.size(1), KVH = k.size(1);
  TORCH_CHECK(q.size(2) == 128 && k.size(2) == 128, op, ": head_dim must be 128");
  TORCH_CHECK(k.size(0) == T && v.sizes() == k.sizes(), op, ": q/k/v disagree on T, KVH or D");
  TORCH_CHECK(KVH > 0 && H % KVH == 0, op, ": H must be a multiple of KVH");
  TORCH_CHECK(k.stride(0) == v.stride(0), op, ": k/v must share the token stride");
  check_dense(op, "grp_seq_start", grp_seq_start, at::kInt);
  const int64_t n_groups = grp_seq_start.numel();
  check_vec(op, "grp_seqlen", grp_seqlen, at::kInt, n_groups);
  check_vec(op, "grp_qpos0", grp_qpos0, at::kInt, n_groups * 8);
  check_one_device(op, out, {q, k, v, grp_seq_start, grp_seqlen, grp_qpos0});
  if (T == 0 || n_groups == 0) return;
  launch_attn_prefill(bf(out), cbf(q), cbf(k), cbf(v), grp_seq_start.data_ptr<int>(),
                      grp_seqlen.data_ptr<int>(), grp_qpos0.data_ptr<int>(), (float)scale,
                      (int)n_groups, (int)H, (int)KVH, (int)q.stride(0), (int)k.stride(0),
                      cur_stream());
}

// The argument checks attn_prefill_paged and attn_prefill_paged_split share;
// `op` names the binding in the messages.
struct PagedPrefillDims { int T, H, KVH, NB, BS, n_seq, n_groups, fp8; const float *ks, *vs; };

static PagedPrefillDims check_paged_prefill(
    const char* op, const Tensor& out, const Tensor& q, const Tensor& k_cache,
    const Tensor& v_cache, const Tensor& block_tables, const Tensor& cu_q, const Tensor& q_start,
    const Tensor& grp_seq, const Tensor& grp_qpos0, const Tensor& k_scale, const Tensor& v_scale) {
  check_rows(op, "q", q);
  check_dense(op, "out", out, at::kBFloat16, q.sizes());
  const CacheDims c = check_cache_pair(op, k_cache, v_cache);
  const int T = q.size(0), H = q.size(1);
  TORCH_CHECK(q.size(2) == 128 && c.D == 128, op, ": head_dim must be 128");
  TORCH_CHECK(c.KVH > 0 && H % c.KVH == 0, op, ": H must be a multiple of KVH");
  check_dense(op, "q_start", q_start, at::kInt);
  const int n_seq = q_start.numel();
  TORCH_CHECK(n_seq >= 1, op, ": needs at least one sequence");
  check_vec(op, "cu_q", cu_q, at::kInt, n_seq + 1);
  check_dense(op, "block_tables", block_tables, at::kInt);
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == n_seq && block_tables.size(1) >= 1,
              op, ": block_tables must be [n_seq, max_blocks]");
  check_dense(op, "grp_seq", grp_seq, at::kInt);
  const int n_groups = grp_seq.numel();
  check_vec(op, "grp_qpos0", grp_qpos0, at::kInt, (int64_t)n_groups * 8);
  const auto [ks, vs] = kv_scales(op, k_cache, k_scale, v_scale);
  check_one_device(op, out, {q, k_cache, v_cache, block_tables, cu_q, q_start, grp_seq, grp_qpos0,
                             k_scale, v_scale});
  return {T, H, (int)c.KVH, (int)c.NB, (int)c.BS, n_seq, n_groups, c.fp8, ks, vs};
}

// Paged (append / extend) prefill attention: new tokens packed at rows
// cu_q[s]..cu_q[s+1] attend causally to the q_start[s] keys already cached
// plus themselves, all read through block_tables[s] (one row per sequence).
// grp_seq [G] / grp_qpos0 [G*8] are the per-workgroup q-tiles of
// ops.build_paged_prefill, which also checks q_start + q_len against the
// table width on the host.
void attn_prefill_paged(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables,
                        Tensor cu_q, Tensor q_start, Tensor grp_seq, Tensor grp_qpos0,
                        double scale, Tensor k_scale, Tensor v_scale) {
  const PagedPrefillDims d = check_paged_prefill(
      "attn_prefill_paged", out, q, k_cache, v_cache, block_tables, cu_q, q_start, grp_seq,
      grp_qpos0, k_scale, v_scale);
  if (d.T == 0 || d.n_groups == 0) return;
  launch_attn_prefill_paged(
      bf(out), cbf(q), k_cache.data_ptr(), v_cache.data_ptr(), d.ks, d.vs,
      block_tables.data_ptr<int>(), cu_q.data_ptr<int>(), q_start.data_ptr<int>(),
      grp_seq.data_ptr<int>(), grp_qpos0.data_ptr<int>(), (float)scale, d.n_seq, d.T, d.H,
      d.KVH, d.NB, d.BS, (int)block_tables.size(1), (int)q.stride(0), d.n_groups, d.fp8,
      cur_stream());
}

// attn_prefill_paged with the keys of some sequences split across workgroups
// (ops.build_paged_prefill(key_splits=...)): grp_krange [G*2] is each
// workgroup's key range, grp_split [G] its split index (-1: the sequence is
// unsplit and the workgroup writes out directly), seq_nsplit / seq_ws_base
// [n_seq] the sequence's split count and first workspace slot. part_o
// [>= ws_rows, H, 128] and part_ml [>= ws_rows, H, 2] (fp32) take the
// partials, which a second kernel merges into out. ws_rows and max_splits are
// the plan's slot count and largest split count.
void attn_prefill_paged_split(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache,
                              Tensor block_tables, Tensor cu_q, Tensor q_start, Tensor grp_seq,
                              Tensor grp_qpos0, Tensor grp_krange, Tensor grp_split,
                              Tensor seq_nsplit, Tensor seq_ws_base, Tensor part_o,
                              Tensor part_ml, int64_t ws_rows, int64_t max_splits, double scale,
                              Tensor k_scale, Tensor v_scale) {
  const char* op = "attn_prefill_paged_split";
  const PagedPrefillDims d = check_paged_prefill(
      op, out, q, k_cache, v_cache, block_tables, cu_q, q_start, grp_seq, grp_qpos0, k_scale,
      v_scale);
  check_vec(op, "grp_krange", grp_krange, at::kInt, (int64_t)d.n_groups * 2);
  check_vec(op, "grp_split", grp_split, at::kInt, d.n_groups);
  check_vec(op, "seq_nsplit", seq_nsplit, at::kInt, d.n_seq);
  check_vec(op, "seq_ws_base", seq_ws_base, at::kInt, d.n_seq);
  TORCH_CHECK(max_splits >= 2 && max_splits <= 64, op, ": max_splits must be 2..64");
  TORCH_CHECK(ws_rows >= 1 && ws_rows <= (int64_t)d.T * max_splits,
              op, ": ws_rows must be 1..T*max_splits");
  auto ws_ok = [&](const Tensor& t, int64_t last) {
    return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat && t.dim() == 3 &&
           t.size(0) >= ws_rows && t.size(1) == d.H && t.size(2) == last && aligned(t, 16);
  };
  TORCH_CHECK(ws_ok(part_o, 128) && ws_ok(part_ml, 2),
              op, ": part_o / part_ml must be contiguous fp32 "
              "[>= ws_rows, H, 128] / [>= ws_rows, H, 2]");
  if (d.T == 0 || d.n_groups == 0) return;
  launch_attn_prefill_paged_split(
      bf(out), cbf(q), k_cache.data_ptr(), v_cache.data_ptr(), d.ks, d.vs,
      block_tables.data_ptr<int>(), cu_q.data_ptr<int>(), q_start.data_ptr<int>(),
      grp_seq.data_ptr<int>(), grp_qpos0.data_ptr<int>(), grp_krange.data_ptr<int>(),
      grp_split.data_ptr<int>(), seq_nsplit.data_ptr<int>(), seq_ws_base.data_ptr<int>(),
      part_o.data_ptr<float>(), part_ml.data_ptr<float>(), (int)ws_rows, (int)max_splits,
      (float)scale, d.n_seq, d.T, d.H, d.KVH, d.NB, d.BS, (int)block_tables.size(1),
      (int)q.stride(0), d.n_groups, d.fp8, cur_stream());
}

// --- sampling (sampling.hip) -----------------------------------------------------

// The arguments sample and sample_fsm share: logits fp32 [B, V]; tokens,
// logprobs and the five per-row parameters dense [B] on its device. Returns
// {B, V}.
static std::pair<int, int> check_sample(const char* op, const Tensor& tokens,
                                        const Tensor& logprobs, const Tensor& logits,
                                        const Tensor& temperatures, const Tensor& top_ps,
                                        const Tensor& top_ks, const Tensor& seeds,
                                        const Tensor& steps) {
  check_dense(op, "logits", logits, at::kFloat);
  TORCH_CHECK(logits.dim() == 2, op, ": logits must be contiguous fp32 [B, V] on GPU");
  const int64_t B = logits.size(0);
  check_vec(op, "tokens", tokens, at::kLong, B);
  check_vec(op, "logprobs", logprobs, at::kFloat, B);
  check_vec(op, "temperatures", temperatures, at::kFloat, B);
  check_vec(op, "top_ps", top_ps, at::kFloat, B);
  check_vec(op, "top_ks", top_ks, at::kInt, B);
  check_vec(op, "seeds", seeds, at::kLong, B);
  check_vec(op, "steps", steps, at::kLong, B);
  check_one_device(op, logits, {tokens, logprobs, temperatures, top_ps, top_ks, seeds, steps});
  return {(int)B, (int)logits.size(1)};
}

// mask: int32 [B, ceil(V/32)] allowed-token words, dbg: fp32 [B, 16]
// diagnostics; an empty tensor for "none" of either.
void sample(Tensor tokens, Tensor logprobs, Tensor logits, Tensor temperatures, Tensor top_ps,
            Tensor top_ks, Tensor seeds, Tensor steps, Tensor mask, Tensor dbg) {
  const char* op = "sample";
  const auto [B, V] = check_sample(op, tokens, logprobs, logits, temperatures, top_ps, top_ks,
                                   seeds, steps);
  if (mask.numel() > 0) check_dense(op, "mask", mask, at::kInt, {B, (V + 31) / 32});
  if (dbg.numel() > 0) check_dense(op, "dbg", dbg, at::kFloat, {B, 16});
  check_one_device(op, logits, {mask, dbg});
  if (B == 0) return;
  launch_sample(tokens.data_ptr<int64_t>(), logprobs.data_ptr<float>(), logits.data_ptr<float>(),
                temperatures.data_ptr<float>(), top_ps.data_ptr<float>(), top_ks.data_ptr<int>(),
                seeds.data_ptr<int64_t>(), steps.data_ptr<int64_t>(),
                mask.numel() ? reinterpret_cast<const uint32_t*>(mask.data_ptr<int>()) : nullptr,
                B, V, dbg.numel() ? dbg.data_ptr<float>() : nullptr, cur_stream());
}

// Constrained sampling with the DFA state on the device: `tabs` [B, 6] holds
// per-stream device addresses of the constraint tables (the caller keeps the
// tables alive past the launch); `fsm_state` [B] is advanced in place.
void sample_fsm(Tensor tokens, Tensor logprobs, Tensor logits, Tensor temperatures, Tensor top_ps,
                Tensor top_ks, Tensor seeds, Tensor steps, Tensor fsm_state, Tensor tabs,
                int64_t eos_id) {
  const char* op = "sample_fsm";
  const auto [B, V] = check_sample(op, tokens, logprobs, logits, temperatures, top_ps, top_ks,
                                   seeds, steps);
  check_dense(op, "fsm_state", fsm_state, at::kInt, {B});
  check_dense(op, "tabs", tabs, at::kLong, {B, 6});
  check_one_device(op, logits, {fsm_state, tabs});
  TORCH_CHECK(eos_id >= -1 && eos_id < V, op, ": eos_id out of range");
  if (B == 0) return;
  launch_sample_fsm(tokens.data_ptr<int64_t>(), logprobs.data_ptr<float>(),
                    logits.data_ptr<float>(), temperatures.data_ptr<float>(),
                    top_ps.data_ptr<float>(), top_ks.data_ptr<int>(), seeds.data_ptr<int64_t>(),
                    steps.data_ptr<int64_t>(), fsm_state.data_ptr<int>(),
                    tabs.data_ptr<int64_t>(), (int)eos_id, B, V, cur_stream());
}

// D[32,32] = A[32,16] x B[16,32], verifying the fragment maps the attention
// kernels assume for v_mfma_f32_32x32x16_bf16 (mfma_selftest.hip).
Tensor mfma_selftest(Tensor A, Tensor B) {
  check_dense("mfma_selftest", "A", A, at::kBFloat16, {32, 16});
  check_dense("mfma_selftest", "B", B, at::kBFloat16, {16, 32});
  check_one_device("mfma_selftest", A, {B});
  auto D = torch::empty({32, 32}, torch::dtype(torch::kFloat).device(A.device()));
  launch_mfma_selftest(D.data_ptr<float>(), cbf(A), cbf(B), cur_stream());
  return D;
}

// --- all-reduce (allreduce.hip) --------------------------------------------------

// In-place sum across up to 8 same-shaped bf16 buffers on one GPU: every
// "peer" buffer ends holding the fp32-accumulated sum. The single-GPU form of
// the one-shot all-reduce, kept for the numerics tests; ranks in separate
// processes go through ipc_allreduce_* below.
void one_shot_allreduce(std::vector<Tensor> bufs) {
  const char* op = "one_shot_allreduce";
  TORCH_CHECK(!bufs.empty() && bufs.size() <= 8, op, ": 1..8 peer buffers");
  const auto numel = bufs[0].numel();
  TORCH_CHECK(numel % 8 == 0, op, ": numel must be a multiple of 8 (16B vector path)");
  const void* srcs[8];
  void* dsts[8];
  for (size_t r = 0; r < bufs.size(); ++r) {
    check_vec(op, "every peer buffer", bufs[r], at::kBFloat16, numel);
    TORCH_CHECK(aligned(bufs[r], 16) && bufs[r].device() == bufs[0].device(),
                op, ": peer buffers must be 16-byte aligned on one device");
    srcs[r] = dsts[r] = bufs[r].data_ptr();
  }
  if (numel == 0) return;
  launch_one_shot_allreduce(srcs, dsts, (int)bufs.size(), (long)numel, /*write_all=*/1,
                            cur_stream());
}

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

// An empty call still goes through ipc_ar_run: the ranks signal each other
// there, and that exchange stays what it was.
void ipc_allreduce_run(int64_t ctx, Tensor inp, Tensor out) {
  check_dense("ipc_allreduce_run", "inp", inp, at::kBFloat16);
  check_vec("ipc_allreduce_run", "out", out, at::kBFloat16, inp.numel());
  check_one_device("ipc_allreduce_run", out, {inp});
  int rc = ipc_ar_run(reinterpret_cast<void*>(ctx), inp.data_ptr(), out.data_ptr(),
                      (long)inp.numel(), cur_stream());
  TORCH_CHECK(rc == 0, "ipc_ar_run failed rc=", rc);
}

void ipc_allreduce_destroy(int64_t ctx) {
  ipc_ar_destroy(reinterpret_cast<void*>(ctx));
}

// --- grouped MoE expert GEMMs (moe.hip) --------------------------------------

// Expert weights [E, N, K]: bf16 with an empty `scale`, or e4m3 with fp32
// per-channel scales [E, N]. Returns the scale pointer (nullptr for bf16).
static const float* moe_weight_scale(const Tensor& w, const Tensor& scale) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.dim() == 3, "expert weights must be contiguous [E, N, K] on GPU");
  if (scale.numel() == 0) {
    TORCH_CHECK(w.scalar_type() == at::kBFloat16, "expert weights without scales must be bf16");
    return nullptr;
  }
  TORCH_CHECK(w.scalar_type() == at::kFloat8_e4m3fn, "expert weights with scales must be e4m3");
  check_dense("grouped MoE", "scale", scale, at::kFloat, {w.size(0), w.size(1)});
  TORCH_CHECK(aligned(w, 16), "e4m3 expert weights must be 16-byte aligned");
  return scale.data_ptr<float>();
}

void moe_gateup(Tensor act, Tensor x, Tensor w, Tensor scale, Tensor sorted_ids,
                Tensor pad_offsets, Tensor zeros) {
  const char* op = "moe_gateup";
  check_dense(op, "act", act, at::kBFloat16);
  check_dense(op, "x", x, at::kBFloat16);
  check_dense(op, "zeros", zeros, at::kBFloat16);
  TORCH_CHECK(act.dim() == 2 && x.dim() == 2, op, ": act and x must be 2-D");
  const float* sc = moe_weight_scale(w, scale);
  const int64_t E = w.size(0), IN = w.size(1) / 2, K = w.size(2);
  check_dense(op, "sorted_ids", sorted_ids, at::kInt, {act.size(0)});
  check_dense(op, "pad_offsets", pad_offsets, at::kInt, {E + 1});
  check_one_device(op, act, {x, w, scale, zeros, sorted_ids, pad_offsets});
  TORCH_CHECK(IN % 64 == 0 && K % 64 == 0, op, ": IN % 64, K % 64 required");
  TORCH_CHECK(act.size(1) == IN && x.size(1) == K && zeros.numel() >= K,
              op, ": act must be [S, IN], x [T, K], zeros at least K long");
  TORCH_CHECK(act.size(0) % 128 == 0, op, ": sorted rows must be padded to 128");
  if (act.size(0) == 0) return;
  launch_moe_gateup(act.data_ptr(), x.data_ptr(), w.data_ptr(), sc, sorted_ids.data_ptr<int>(),
                    pad_offsets.data_ptr<int>(), zeros.data_ptr(), (int)E, (int)IN, (int)K,
                    cur_stream());
}

void moe_down(Tensor y, Tensor act, Tensor w, Tensor scale, Tensor pad_offsets) {
  const char* op = "moe_down";
  check_dense(op, "y", y, at::kBFloat16);
  check_dense(op, "act", act, at::kBFloat16);
  TORCH_CHECK(y.dim() == 2 && act.dim() == 2, op, ": y and act must be 2-D");
  const float* sc = moe_weight_scale(w, scale);
  const int64_t E = w.size(0), H = w.size(1), IN = w.size(2);
  check_dense(op, "pad_offsets", pad_offsets, at::kInt, {E + 1});
  check_one_device(op, y, {act, w, scale, pad_offsets});
  TORCH_CHECK(H % 64 == 0 && IN % 64 == 0, op, ": H % 64, IN % 64 required");
  TORCH_CHECK(y.size(1) == H && act.size(1) == IN, op, ": y must be [S, H] and act [S, IN]");
  TORCH_CHECK(y.size(0) == act.size(0), op, ": y and act must have the same sorted rows");
  TORCH_CHECK(y.size(0) % 128 == 0, op, ": sorted rows must be padded to 128");
  if (y.size(0) == 0) return;
  launch_moe_down(y.data_ptr(), act.data_ptr(), w.data_ptr(), sc, pad_offsets.data_ptr<int>(),
                  (int)E, (int)H, (int)IN, cur_stream());
}

// --- batched Levenshtein (levenshtein.hip) -----------------------------------

Tensor levenshtein_pairs(Tensor chars, Tensor lens, Tensor pair_i, Tensor pair_j) {
  const char* op = "levenshtein_pairs";
  check_dense(op, "chars", chars, at::kByte);
  TORCH_CHECK(chars.dim() == 2 && chars.size(1) == 64,
              op, ": chars must be contiguous uint8 [N, 64] on GPU");
  check_vec(op, "lens", lens, at::kInt, chars.size(0));
  check_dense(op, "pair_i", pair_i, at::kInt);
  const int64_t P = pair_i.numel();
  check_vec(op, "pair_j", pair_j, at::kInt, P);
  check_one_device(op, chars, {lens, pair_i, pair_j});
  auto out = torch::empty({P}, torch::dtype(torch::kInt).device(chars.device()));
  if (P == 0) return out;
  launch_levenshtein(out.data_ptr<int>(), chars.data_ptr<unsigned char>(), lens.data_ptr<int>(),
                     pair_i.data_ptr<int>(), pair_j.data_ptr<int>(), (long)P, cur_stream());
  return out;
}

// --- weight-only fp8 GEMM (linear_fp8w.hip) ------------------------------------

// q e4m3 [N, K] with fp32 per-row scales [N]
static void check_fp8w(const Tensor& q, const Tensor& scale) {
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() && q.dim() == 2 &&
              q.scalar_type() == at::kFloat8_e4m3fn, "q must be contiguous e4m3 [N, K] on GPU");
  check_vec("fp8w", "scale", scale, at::kFloat, q.size(0));
}

// out[M, N] = bf16((x @ q^T) * scale + bias); bias: bf16 [N] or an empty tensor.
// Takes 1 <= M <= 256, K % 64 == 0, N % 16 == 0, x with unit inner stride and
// a 16-byte-aligned row stride >= K (ops.linear_fp8w routes everything else
// through dequant_fp8w).
void linear_fp8w(Tensor out, Tensor x, Tensor q, Tensor scale, Tensor bias) {
  const char* op = "linear_fp8w";
  check_fp8w(q, scale);
  const int64_t M = x.size(0), K = x.size(1), N = q.size(0);
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 &&
              x.stride(1) == 1 && x.stride(0) >= K && x.stride(0) % 8 == 0 && aligned(x, 16),
              op, ": x must be a bf16 [M, K] row view with 16-byte-aligned rows");
  TORCH_CHECK(q.size(1) == K, op, ": x and q disagree on K");
  TORCH_CHECK(M >= 1 && M <= 256 && K % 64 == 0 && N % 16 == 0,
              op, ": needs 1 <= M <= 256, K % 64 == 0, N % 16 == 0; got M=", M,
              " N=", N, " K=", K);
  check_dense(op, "out", out, at::kBFloat16, {M, N});
  TORCH_CHECK(aligned(q, 16) && aligned(scale, 16) && aligned(out, 8),
              op, ": q/scale must be 16-byte aligned, out 8-byte aligned");
  const void* bptr = nullptr;
  if (bias.numel() > 0) {
    check_vec(op, "bias", bias, at::kBFloat16, N);
    TORCH_CHECK(aligned(bias, 8), op, ": bias must be 8-byte aligned");
    bptr = bias.data_ptr();
  }
  const int n_cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  int mt = 1, splitk = 1;
  linear_fp8w_plan((int)M, (int)N, (int)K, n_cus, &mt, &splitk);
  float* slabs = nullptr;
  Tensor ws;
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
void linear_fp8w_batched(Tensor out, Tensor x, Tensor q, Tensor scale) {
  const char* op = "linear_fp8w_batched";
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() && q.dim() == 3 &&
              q.scalar_type() == at::kFloat8_e4m3fn,
              op, ": q must be contiguous e4m3 [E, N, K] on GPU");
  const int64_t E = q.size(0), N = q.size(1), K = q.size(2);
  check_dense(op, "scale", scale, at::kFloat, {E, N});
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && (x.dim() == 2 || x.dim() == 3),
              op, ": x must be bf16 [M, K] or [E, M, K] on GPU");
  const bool shared = x.dim() == 2;
  const int64_t M = x.size(shared ? 0 : 1);
  const int64_t x_stride = x.stride(shared ? 0 : 1);
  const int64_t x_bstride = shared ? 0 : x.stride(0);
  TORCH_CHECK(x.size(-1) == K && (shared || x.size(0) == E), op, ": x and q disagree on E or K");
  TORCH_CHECK(E >= 1 && E <= 1024 && M >= 1 && M <= 256 && K % 64 == 0 && N % 16 == 0,
              op, ": needs 1 <= E <= 1024, 1 <= M <= 256, K % 64 == 0, "
              "N % 16 == 0; got E=", E, " M=", M, " N=", N, " K=", K);
  TORCH_CHECK(x.stride(-1) == 1 && x_stride >= K && x_stride % 8 == 0 && x_bstride % 8 == 0 &&
              aligned(x, 16),
              op, ": x needs unit inner stride and 16-byte-aligned rows and experts");
  check_dense(op, "out", out, at::kBFloat16, {E, M, N});
  TORCH_CHECK(aligned(q, 16) && aligned(scale, 16) && aligned(out, 8),
              op, ": q/scale must be 16-byte aligned, out 8-byte aligned");
  const int n_cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  int mt = 1, splitk = 1;
  linear_fp8w_batched_plan((int)E, (int)M, (int)N, (int)K, n_cus, &mt, &splitk);
  float* slabs = nullptr;
  Tensor ws;
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
void dequant_fp8w(Tensor w, Tensor q, Tensor scale) {
  const char* op = "dequant_fp8w";
  check_fp8w(q, scale);
  check_dense(op, "w", w, at::kBFloat16);
  TORCH_CHECK(w.numel() >= q.numel(), op, ": scratch smaller than the weight");
  TORCH_CHECK(q.size(1) % 16 == 0, op, ": K must be a multiple of 16");
  TORCH_CHECK(aligned(q, 16) && aligned(w, 16), op, ": q and w must be 16-byte aligned");
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
