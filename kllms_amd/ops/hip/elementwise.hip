// Memory-bound elementwise / normalization kernels for gfx950.
//
// All of these are HBM-bandwidth-bound: the design rules applied are
// G13 (vectorize bf16 as 8-element/16-byte lane loads), G11 (grid-stride with
// a capped grid), and fusion (residual-add folded into RMSNorm; cos/sin for
// RoPE precomputed on host — Appendix B: on-device trig turns memory-bound
// into VALU-bound).

#include "launch.h"

#include <algorithm>

// --------------------------------------------------------------------------
// RMSNorm: one block per row, row length N (multiple of 8), bf16 in/out.
// y = x / sqrt(mean(x^2) + eps) * w      (fp32 accumulation)
// --------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256) rmsnorm_kernel(
    bf16_t* __restrict__ out, const bf16_t* __restrict__ in,
    const bf16_t* __restrict__ w, int n, float eps) {
  __shared__ float red[16];
  const int row = blockIdx.x;
  const bf16x8_vec* inv = reinterpret_cast<const bf16x8_vec*>(in + (int64_t)row * n);
  bf16x8_vec* outv = reinterpret_cast<bf16x8_vec*>(out + (int64_t)row * n);
  const bf16x8_vec* wv = reinterpret_cast<const bf16x8_vec*>(w);
  const int nvec = n / 8;

  float ss = 0.0f;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    bf16x8_vec v = inv[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf16_to_f32(v[j]);
      ss += f * f;
    }
  }
  ss = block_reduce_sum<4>(ss, red);
  const float inv_rms = rsqrtf(ss / n + eps);

  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    bf16x8_vec v = inv[i];
    bf16x8_vec wv8 = wv[i];
    bf16x8_vec o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = f32_to_bf16(bf16_to_f32(v[j]) * inv_rms * bf16_to_f32(wv8[j]));
    outv[i] = o;
  }
}

// --------------------------------------------------------------------------
// Fused residual-add + RMSNorm: residual += x (written back), y = rmsnorm(residual)
// --------------------------------------------------------------------------
// ss + round(f * f): the square is rounded on its own and then added, the
// form every build of this kernel has used (v_pk_mul_f32 + v_add_f32). Written
// out so that both paths below keep it whatever the compiler would contract.
__device__ __forceinline__ float add_square(float ss, float f) {
#pragma clang fp contract(off)
  const float sq = f * f;
  return ss + sq;
}

// residual' = bf16(x + residual) of one 8-wide vector; returns the vector and
// adds its squares to ss in element order.
__device__ __forceinline__ bf16x8_vec add_round_vec(bf16x8_vec a, bf16x8_vec b, float& ss) {
  bf16x8_vec s;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f = bf16_to_f32(a[j]) + bf16_to_f32(b[j]);
    s[j] = f32_to_bf16(f);
    ss = add_square(ss, bf16_to_f32(s[j]));  // accumulate on the bf16-rounded sum
  }
  return s;
}

__device__ __forceinline__ bf16x8_vec scale_vec(bf16x8_vec s, bf16x8_vec w8, float inv_rms) {
  bf16x8_vec o;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    o[j] = f32_to_bf16(bf16_to_f32(s[j]) * inv_rms * bf16_to_f32(w8[j]));
  return o;
}

#define ADD_RMSNORM_REG_VECS 4   // summed vectors a thread keeps in registers

extern "C" __global__ void __launch_bounds__(256) fused_add_rmsnorm_kernel(
    bf16_t* __restrict__ out, const bf16_t* __restrict__ x,
    bf16_t* __restrict__ residual, const bf16_t* __restrict__ w, int n, float eps) {
  __shared__ float red[16];
  const int row = blockIdx.x;
  const bf16x8_vec* xv = reinterpret_cast<const bf16x8_vec*>(x + (int64_t)row * n);
  bf16x8_vec* rv = reinterpret_cast<bf16x8_vec*>(residual + (int64_t)row * n);
  bf16x8_vec* outv = reinterpret_cast<bf16x8_vec*>(out + (int64_t)row * n);
  const bf16x8_vec* wv = reinterpret_cast<const bf16x8_vec*>(w);
  const int nvec = n / 8;

  float ss = 0.0f;
  if (nvec <= ADD_RMSNORM_REG_VECS * (int)blockDim.x) {
    // Register path (n <= 8192 at 256 threads): a thread's summed vectors stay
    // in registers across the reduction, so the second pass reads nothing
    // back, and the weight loads are issued with the inputs, ahead of the
    // barrier. Same vectors per thread, same order of additions into ss.
    bf16x8_vec s[ADD_RMSNORM_REG_VECS], wr[ADD_RMSNORM_REG_VECS];
#pragma unroll
    for (int u = 0; u < ADD_RMSNORM_REG_VECS; ++u) {
      const int i = threadIdx.x + u * blockDim.x;
      if (i < nvec) {
        bf16x8_vec a = xv[i];
        bf16x8_vec b = rv[i];
        wr[u] = wv[i];
        s[u] = add_round_vec(a, b, ss);
        rv[i] = s[u];
      }
    }
    ss = block_reduce_sum<4>(ss, red);
    const float inv_rms = rsqrtf(ss / n + eps);
#pragma unroll
    for (int u = 0; u < ADD_RMSNORM_REG_VECS; ++u) {
      const int i = threadIdx.x + u * blockDim.x;
      if (i < nvec) outv[i] = scale_vec(s[u], wr[u], inv_rms);
    }
    return;
  }

  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    bf16x8_vec a = xv[i];
    bf16x8_vec b = rv[i];
    rv[i] = add_round_vec(a, b, ss);
  }
  ss = block_reduce_sum<4>(ss, red);
  const float inv_rms = rsqrtf(ss / n + eps);

  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    bf16x8_vec s = rv[i];
    bf16x8_vec wv8 = wv[i];
    bf16x8_vec o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = f32_to_bf16(bf16_to_f32(s[j]) * inv_rms * bf16_to_f32(wv8[j]));
    outv[i] = o;
  }
}

// --------------------------------------------------------------------------
// SwiGLU activation: out = silu(gate) * up, bf16, grid-stride, 8-wide.
// --------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256) silu_mul_kernel(
    bf16_t* __restrict__ out, const bf16_t* __restrict__ gate,
    const bf16_t* __restrict__ up, int64_t nvec, int ncols_vec, int row_stride_vec) {
  // gate/up are [rows, ncols] row-views with a free row stride (the fused
  // gate_up GEMM output), out is contiguous [rows, ncols]
  bf16x8_vec* ov = reinterpret_cast<bf16x8_vec*>(out);
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / ncols_vec;
    const int64_t col = i % ncols_vec;
    const int64_t src = row * row_stride_vec + col;
    bf16x8_vec g = reinterpret_cast<const bf16x8_vec*>(gate)[src];
    bf16x8_vec u = reinterpret_cast<const bf16x8_vec*>(up)[src];
    bf16x8_vec o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gf = bf16_to_f32(g[j]);
      float s = gf / (1.0f + __expf(-gf));
      o[j] = f32_to_bf16(s * bf16_to_f32(u[j]));
    }
    ov[i] = o;
  }
}

// --------------------------------------------------------------------------
// RoPE (Llama rotate-half): in-place on q [T, H, D] and k [T, KVH, D].
// cos_sin: [max_pos, D] fp32, cos in [0, D/2), sin in [D/2, D).
// Grid: (T, H + KVH); block = D/2 threads (one lane per rotation pair).
// --------------------------------------------------------------------------
extern "C" __global__ void rope_kernel(
    bf16_t* __restrict__ q, bf16_t* __restrict__ k,
    const int64_t* __restrict__ positions, const float* __restrict__ cos_sin,
    int num_q_heads, int num_kv_heads, int head_dim, int q_tstride, int k_tstride) {
  const int t = blockIdx.x;
  const int h = blockIdx.y;
  const int i = threadIdx.x;           // pair index in [0, D/2)
  const int half = head_dim / 2;
  if (i >= half) return;
  const int64_t pos = positions[t];
  const float c = cos_sin[pos * head_dim + i];
  const float s = cos_sin[pos * head_dim + half + i];
  bf16_t* base;
  if (h < num_q_heads) {
    base = q + (int64_t)t * q_tstride + h * head_dim;
  } else {
    base = k + (int64_t)t * k_tstride + (h - num_q_heads) * head_dim;
  }
  float x1 = bf16_to_f32(((const short*)base)[i]);
  float x2 = bf16_to_f32(((const short*)base)[half + i]);
  ((short*)base)[i] = f32_to_bf16(x1 * c - x2 * s);
  ((short*)base)[half + i] = f32_to_bf16(x2 * c + x1 * s);
}

// --------------------------------------------------------------------------
// Paged-KV scatter: k/v [T, KVH, D] -> caches [NB, KVH, BS, D] at flat slots.
// Grid-stride over T*KVH*(D/8); 16-byte lane copies.
// --------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256) store_kv_kernel(
    const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    bf16_t* __restrict__ k_cache, bf16_t* __restrict__ v_cache,
    const int64_t* __restrict__ slots, int num_tokens, int kv_heads,
    int head_dim, int block_size, int kv_tstride) {
  const int dvec = head_dim / 8;
  const int64_t total = (int64_t)num_tokens * kv_heads * dvec;
  for (int64_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int dv = idx % dvec;
    const int g = (idx / dvec) % kv_heads;
    const int t = idx / ((int64_t)dvec * kv_heads);
    const int64_t slot = slots[t];
    const int64_t blk = slot / block_size;
    const int off = slot % block_size;
    const bf16x8_vec* src_k =
        reinterpret_cast<const bf16x8_vec*>(k + (int64_t)t * kv_tstride + g * head_dim) + dv;
    const bf16x8_vec* src_v =
        reinterpret_cast<const bf16x8_vec*>(v + (int64_t)t * kv_tstride + g * head_dim) + dv;
    int64_t dst_off = ((blk * kv_heads + g) * block_size + off) * head_dim;
    reinterpret_cast<bf16x8_vec*>(k_cache + dst_off)[dv] = *src_k;
    reinterpret_cast<bf16x8_vec*>(v_cache + dst_off)[dv] = *src_v;
  }
}

// fp8 (e4m3) variant of the paged-KV scatter with PER-ROW dequant scales:
// one 64-lane wave per (token, kv_head) row computes s = max(amax|row|/448,
// 1e-8) over the row's K (and V) values, stores the scales to
// k_scale/v_scale [NB, KVH, BS] and quantizes x/s into the 1-byte caches —
// outlier rows in real checkpoints no longer saturate e4m3's +-448 range.
// T*KVH rows per call is tiny next to the attention reads, so a plain
// strided (non-vectorized) load pattern is fine here.
extern "C" __global__ void __launch_bounds__(256) store_kv_fp8_kernel(
    const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    unsigned char* __restrict__ k_cache, unsigned char* __restrict__ v_cache,
    float* __restrict__ k_scale, float* __restrict__ v_scale,
    const int64_t* __restrict__ slots, int num_tokens, int kv_heads,
    int head_dim, int block_size, int kv_tstride) {
  const int64_t rows = (int64_t)num_tokens * kv_heads;
  const int lane = threadIdx.x & 63;
  for (int64_t row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows;
       row += (int64_t)gridDim.x * 4) {
    const int g = row % kv_heads;
    const int t = row / kv_heads;
    const int64_t slot = slots[t];
    const int64_t blk = slot / block_size;
    const int off = slot % block_size;
    const bf16_t* src_k = k + (int64_t)t * kv_tstride + g * head_dim;
    const bf16_t* src_v = v + (int64_t)t * kv_tstride + g * head_dim;
    float amax_k = 0.f, amax_v = 0.f;
    for (int d = lane; d < head_dim; d += 64) {
      amax_k = fmaxf(amax_k, fabsf(bf16_to_f32(((const short*)src_k)[d])));
      amax_v = fmaxf(amax_v, fabsf(bf16_to_f32(((const short*)src_v)[d])));
    }
    const float sk = fmaxf(wave_reduce_max(amax_k) * (1.0f / 448.0f), 1e-8f);
    const float sv = fmaxf(wave_reduce_max(amax_v) * (1.0f / 448.0f), 1e-8f);
    const int64_t srow = (blk * kv_heads + g) * block_size + off;
    if (lane == 0) { k_scale[srow] = sk; v_scale[srow] = sv; }
    const float isk = 1.0f / sk, isv = 1.0f / sv;
    unsigned char* dst_k = k_cache + srow * head_dim;
    unsigned char* dst_v = v_cache + srow * head_dim;
    for (int d = lane; d < head_dim; d += 64) {
      dst_k[d] = f32_to_fp8(bf16_to_f32(((const short*)src_k)[d]) * isk);
      dst_v[d] = f32_to_fp8(bf16_to_f32(((const short*)src_v)[d]) * isv);
    }
  }
}

// --------------------------------------------------------------------------
// RoPE + paged-KV store in one launch: rotates q and k in place exactly as
// rope_kernel does, then writes the rotated (bf16-rounded) k and the untouched
// v into the paged caches at slots[t] -- the bits rope_kernel followed by
// store_kv_kernel / store_kv_fp8_kernel leave behind, without re-reading k.
// One 64-lane wave per (token, head) row, 4 rows of one token per block;
// grid (T, ceil((H + KVH) / 4)). A k-head wave also moves its head's v row.
// Rows that share a slot (padded graph lanes) write the same few bytes in
// any order, which is as harmless as it is with the two kernels.
// --------------------------------------------------------------------------

// The two rotation outputs in the form rope_kernel compiles to (one product
// rounded on its own, the other fused into the sum); written out because the
// compiler's contraction of `x1 * c - x2 * s` is not stable across kernels.
__device__ __forceinline__ float rope_first(float x1, float x2, float c, float s) {
#pragma clang fp contract(off)
  const float p = x2 * s;
  return __builtin_fmaf(x1, c, -p);
}

__device__ __forceinline__ float rope_second(float x1, float x2, float c, float s) {
#pragma clang fp contract(off)
  const float p = x2 * c;
  return __builtin_fmaf(x1, s, p);
}

template <bool FP8>
__device__ __forceinline__ void rope_store_kv_body(
    bf16_t* __restrict__ q, bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    void* __restrict__ k_cache, void* __restrict__ v_cache,
    float* __restrict__ k_scale, float* __restrict__ v_scale,
    const int64_t* __restrict__ positions, const float* __restrict__ cos_sin,
    const int64_t* __restrict__ slots, int num_q_heads, int num_kv_heads, int head_dim,
    int block_size, int q_tstride, int k_tstride, int v_tstride) {
  const int t = blockIdx.x;
  const int h = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (h >= num_q_heads + num_kv_heads) return;   // wave-uniform
  const int half = head_dim / 2;
  const int64_t pos = positions[t];
  const float* cs = cos_sin + pos * head_dim;
  const bool is_k = h >= num_q_heads;
  const int g = h - num_q_heads;
  short* base = reinterpret_cast<short*>(
      is_k ? k + (int64_t)t * k_tstride + g * head_dim : q + (int64_t)t * q_tstride + h * head_dim);

  if (!is_k) {
    for (int i = lane; i < half; i += 64) {
      const float c = cs[i], s = cs[half + i];
      const float x1 = bf16_to_f32(base[i]), x2 = bf16_to_f32(base[half + i]);
      base[i] = f32_to_bf16(rope_first(x1, x2, c, s));
      base[half + i] = f32_to_bf16(rope_second(x1, x2, c, s));
    }
    return;
  }

  const int64_t slot = slots[t];
  const int64_t blk = slot / block_size;
  const int off = slot % block_size;
  const int64_t srow = (blk * num_kv_heads + g) * block_size + off;
  const short* src_v = reinterpret_cast<const short*>(v + (int64_t)t * v_tstride + g * head_dim);

  if (!FP8) {
    short* dst_k = reinterpret_cast<short*>(k_cache) + srow * head_dim;
    for (int i = lane; i < half; i += 64) {
      const float c = cs[i], s = cs[half + i];
      const float x1 = bf16_to_f32(base[i]), x2 = bf16_to_f32(base[half + i]);
      const short r1 = f32_to_bf16(rope_first(x1, x2, c, s));
      const short r2 = f32_to_bf16(rope_second(x1, x2, c, s));
      base[i] = r1;
      base[half + i] = r2;
      dst_k[i] = r1;
      dst_k[half + i] = r2;
    }
    bf16x8_vec* dst_v = reinterpret_cast<bf16x8_vec*>(reinterpret_cast<short*>(v_cache) + srow * head_dim);
    for (int dv = lane; dv < head_dim / 8; dv += 64)
      dst_v[dv] = reinterpret_cast<const bf16x8_vec*>(src_v)[dv];
    return;
  }

  // fp8: the arithmetic of store_kv_fp8_kernel on the rounded k. A lane keeps
  // its first two rotation pairs in registers (all of them up to head_dim
  // 256); beyond that it re-reads the elements it has just written itself.
  float amax_k = 0.f, amax_v = 0.f;
  auto rotate = [&](int i, short& r1, short& r2) {
    const float c = cs[i], s = cs[half + i];
    const float x1 = bf16_to_f32(base[i]), x2 = bf16_to_f32(base[half + i]);
    r1 = f32_to_bf16(rope_first(x1, x2, c, s));
    r2 = f32_to_bf16(rope_second(x1, x2, c, s));
    base[i] = r1;
    base[half + i] = r2;
    amax_k = fmaxf(amax_k, fabsf(bf16_to_f32(r1)));
    amax_k = fmaxf(amax_k, fabsf(bf16_to_f32(r2)));
  };
  short ra1 = 0, ra2 = 0, rb1 = 0, rb2 = 0;
  if (lane < half) rotate(lane, ra1, ra2);
  if (lane + 64 < half) rotate(lane + 64, rb1, rb2);
  for (int i = lane + 128; i < half; i += 64) {
    short r1, r2;
    rotate(i, r1, r2);
  }
  for (int d = lane; d < head_dim; d += 64)
    amax_v = fmaxf(amax_v, fabsf(bf16_to_f32(src_v[d])));
  const float sk = fmaxf(wave_reduce_max(amax_k) * (1.0f / 448.0f), 1e-8f);
  const float sv = fmaxf(wave_reduce_max(amax_v) * (1.0f / 448.0f), 1e-8f);
  if (lane == 0) { k_scale[srow] = sk; v_scale[srow] = sv; }
  const float isk = 1.0f / sk, isv = 1.0f / sv;
  unsigned char* dst_k = reinterpret_cast<unsigned char*>(k_cache) + srow * head_dim;
  unsigned char* dst_v = reinterpret_cast<unsigned char*>(v_cache) + srow * head_dim;
  if (lane < half) {
    dst_k[lane] = f32_to_fp8(bf16_to_f32(ra1) * isk);
    dst_k[half + lane] = f32_to_fp8(bf16_to_f32(ra2) * isk);
  }
  if (lane + 64 < half) {
    dst_k[lane + 64] = f32_to_fp8(bf16_to_f32(rb1) * isk);
    dst_k[half + lane + 64] = f32_to_fp8(bf16_to_f32(rb2) * isk);
  }
  for (int i = lane + 128; i < half; i += 64) {
    dst_k[i] = f32_to_fp8(bf16_to_f32(base[i]) * isk);
    dst_k[half + i] = f32_to_fp8(bf16_to_f32(base[half + i]) * isk);
  }
  for (int d = lane; d < head_dim; d += 64)
    dst_v[d] = f32_to_fp8(bf16_to_f32(src_v[d]) * isv);
}

extern "C" __global__ void __launch_bounds__(256) rope_store_kv_kernel(
    bf16_t* __restrict__ q, bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    bf16_t* __restrict__ k_cache, bf16_t* __restrict__ v_cache,
    const int64_t* __restrict__ positions, const float* __restrict__ cos_sin,
    const int64_t* __restrict__ slots, int num_q_heads, int num_kv_heads, int head_dim,
    int block_size, int q_tstride, int k_tstride, int v_tstride) {
  rope_store_kv_body<false>(q, k, v, k_cache, v_cache, nullptr, nullptr, positions, cos_sin,
                            slots, num_q_heads, num_kv_heads, head_dim, block_size,
                            q_tstride, k_tstride, v_tstride);
}

extern "C" __global__ void __launch_bounds__(256) rope_store_kv_fp8_kernel(
    bf16_t* __restrict__ q, bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    unsigned char* __restrict__ k_cache, unsigned char* __restrict__ v_cache,
    float* __restrict__ k_scale, float* __restrict__ v_scale,
    const int64_t* __restrict__ positions, const float* __restrict__ cos_sin,
    const int64_t* __restrict__ slots, int num_q_heads, int num_kv_heads, int head_dim,
    int block_size, int q_tstride, int k_tstride, int v_tstride) {
  rope_store_kv_body<true>(q, k, v, k_cache, v_cache, k_scale, v_scale, positions, cos_sin,
                           slots, num_q_heads, num_kv_heads, head_dim, block_size,
                           q_tstride, k_tstride, v_tstride);
}

// --------------------------------------------------------------------------
// Host-side launchers (contracts in launch.h). The grid-stride kernels cap
// their grid at ELEM_MAX_GRID blocks (G11).
// --------------------------------------------------------------------------
#define ELEM_THREADS 256
#define ELEM_MAX_GRID 2048
#define ROWS_PER_BLOCK (ELEM_THREADS / WAVE)   // one wave per row: blockIdx * 4 + (threadIdx >> 6)

static int capped_grid(int64_t work_items, int per_block) {
  return (int)std::min<int64_t>((work_items + per_block - 1) / per_block, ELEM_MAX_GRID);
}

extern "C" void launch_rmsnorm(bf16_t* out, const bf16_t* in, const bf16_t* w, int rows, int n,
                               float eps, hipStream_t stream) {
  hipLaunchKernelGGL(rmsnorm_kernel, dim3(rows), dim3(ELEM_THREADS), 0, stream, out, in, w, n, eps);
}

extern "C" void launch_fused_add_rmsnorm(bf16_t* out, const bf16_t* x, bf16_t* residual,
                                         const bf16_t* w, int rows, int n, float eps,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(fused_add_rmsnorm_kernel, dim3(rows), dim3(ELEM_THREADS), 0, stream,
                     out, x, residual, w, n, eps);
}

extern "C" void launch_silu_mul(bf16_t* out, const bf16_t* gate, const bf16_t* up, int64_t rows,
                                int64_t ncols, int64_t row_stride, hipStream_t stream) {
  const int64_t nvec = rows * ncols / 8;
  hipLaunchKernelGGL(silu_mul_kernel, dim3(capped_grid(nvec, ELEM_THREADS)), dim3(ELEM_THREADS),
                     0, stream, out, gate, up, nvec, (int)(ncols / 8), (int)(row_stride / 8));
}

extern "C" void launch_rope(bf16_t* q, bf16_t* k, const int64_t* positions, const float* cos_sin,
                            int T, int num_q_heads, int num_kv_heads, int head_dim,
                            int q_tstride, int k_tstride, hipStream_t stream) {
  // one lane per rotation pair
  hipLaunchKernelGGL(rope_kernel, dim3(T, num_q_heads + num_kv_heads), dim3(head_dim / 2), 0,
                     stream, q, k, positions, cos_sin, num_q_heads, num_kv_heads, head_dim,
                     q_tstride, k_tstride);
}

extern "C" void launch_store_kv(const bf16_t* k, const bf16_t* v, void* k_cache, void* v_cache,
                                float* k_scale, float* v_scale, const int64_t* slots, int T,
                                int num_kv_heads, int head_dim, int block_size, int kv_tstride,
                                int cache_fp8, hipStream_t stream) {
  if (cache_fp8) {
    // per-row quantization: one wave per (token, head) row
    const int grid = capped_grid((int64_t)T * num_kv_heads, ROWS_PER_BLOCK);
    hipLaunchKernelGGL(store_kv_fp8_kernel, dim3(grid), dim3(ELEM_THREADS), 0, stream, k, v,
                       (unsigned char*)k_cache, (unsigned char*)v_cache, k_scale, v_scale, slots,
                       T, num_kv_heads, head_dim, block_size, kv_tstride);
  } else {
    const int grid = capped_grid((int64_t)T * num_kv_heads * (head_dim / 8), ELEM_THREADS);
    hipLaunchKernelGGL(store_kv_kernel, dim3(grid), dim3(ELEM_THREADS), 0, stream, k, v,
                       (bf16_t*)k_cache, (bf16_t*)v_cache, slots, T, num_kv_heads, head_dim,
                       block_size, kv_tstride);
  }
}

extern "C" void launch_rope_store_kv(bf16_t* q, bf16_t* k, const bf16_t* v, void* k_cache,
                                     void* v_cache, float* k_scale, float* v_scale,
                                     const int64_t* positions, const float* cos_sin,
                                     const int64_t* slots, int T, int num_q_heads,
                                     int num_kv_heads, int head_dim, int block_size,
                                     int q_tstride, int k_tstride, int v_tstride, int cache_fp8,
                                     hipStream_t stream) {
  const dim3 grid(T, (num_q_heads + num_kv_heads + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (cache_fp8)
    hipLaunchKernelGGL(rope_store_kv_fp8_kernel, grid, dim3(ELEM_THREADS), 0, stream, q, k, v,
                       (unsigned char*)k_cache, (unsigned char*)v_cache, k_scale, v_scale,
                       positions, cos_sin, slots, num_q_heads, num_kv_heads, head_dim,
                       block_size, q_tstride, k_tstride, v_tstride);
  else
    hipLaunchKernelGGL(rope_store_kv_kernel, grid, dim3(ELEM_THREADS), 0, stream, q, k, v,
                       (bf16_t*)k_cache, (bf16_t*)v_cache, positions, cos_sin, slots,
                       num_q_heads, num_kv_heads, head_dim, block_size, q_tstride, k_tstride,
                       v_tstride);
}
