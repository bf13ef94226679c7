// Shared-prefix ("cascade") decode attention for forked streams, gfx950.
//
// The n streams forked from one prompt all attend to the same prompt K/V.
// attn_decode_partial_t streams that K/V once PER STREAM; this kernel streams
// it once PER GROUP and multiplies it against every member's query rows
// (members x GQA of them) with bf16 MFMA.
//
// It plugs into the existing split-K machinery unchanged: the partials
// buffer [B, KVH, max_chunks, gqa, 130] is indexed by absolute 256-key
// chunks, so this kernel writes the partials of chunks 0..S-1 for every
// member row (same layout and semantics as attn_decode_partial_t: 128
// unnormalised sum(p*v), then m, then l, softmax scale folded into the
// scores), the per-stream kernel skips those chunks (skip_chunks[b]) and
// attn_decode_reduce_kernel merges both sets as it always did. A shared
// chunk is always a full 256 keys: no tail masking, no context lengths.
//
// Grid (n_tiles, KVH, max_chunks), 256 threads. A tile is up to 64 query rows
// of ONE group (tile row R -> member R / gqa, q-head R % gqa; rows past the
// last member are zero-Q padding and never stored). K/V rows are gathered
// through the block table of the tile's FIRST member only.
//
// Per workgroup: the chunk is processed in 2 rounds of 128 keys staged in
// LDS (the attn_mfma.h layouts). The four waves split the KEYS (32 per wave
// per round), never the rows: each wave runs the attn_mfma.h tile core over
// its keys for both 32-row blocks — without defer-max, and unmasked: every
// score is finite — and the four (m, l, o) sets are merged through LDS at the
// end.

#include "attn_mfma.h"
#include "launch.h"

#define SP_THREADS 256
#define SP_TILE_ROWS 64            // query rows per tile (2 MFMA row blocks)
#define SP_ROUND_KEYS 128          // keys staged per barrier round (32 per wave)
#define SP_VT_ROW 136              // shorts: 128 keys + 8 pad (conflict-free b128 reads)
#define SP_O_STRIDE 132            // floats per merged-o row (16B-aligned rows)
#define SP_PART_STRIDE ATTN_DECODE_PART_STRIDE

#define SP_STAGE_BYTES (SP_ROUND_KEYS * ATTN_K_ROW_BYTES + 128 * SP_VT_ROW * 2)   // 67584
#define SP_MERGE_BYTES (4 * 32 * SP_O_STRIDE * 4)                              // 67584
#define SP_LDS_BYTES ((SP_STAGE_BYTES > SP_MERGE_BYTES ? SP_STAGE_BYTES : SP_MERGE_BYTES) + 4 * 32 * 2 * 4)

// 2 workgroups per CU (<= 256 registers, 2 x 67 KB of LDS): one stages while
// the other computes
template <bool FP8>
__global__ __launch_bounds__(SP_THREADS, 2) void attn_decode_shared_t(
    float* __restrict__ partials,        // [B, KVH, max_chunks, gqa, 130]
    const bf16_t* __restrict__ q,        // [B, H, 128], row stride q_tstride
    const char* __restrict__ k_cache,    // [NB, KVH, BS, 128], bf16 or fp8
    const char* __restrict__ v_cache,
    const float* __restrict__ k_scale,   // [NB, KVH, BS] per-row dequant (FP8 only)
    const float* __restrict__ v_scale,
    const int* __restrict__ block_tables,   // [B, max_blocks]
    const int* __restrict__ tile_rows,      // [n_tiles, 64] member batch rows
    const int* __restrict__ tile_nmembers,  // [n_tiles]
    const int* __restrict__ tile_chunks,    // [n_tiles] shared 256-key chunks
    float scale, int B, int gqa, int num_kv_heads, int num_blocks,
    int block_size, int max_blocks, int max_chunks, int q_tstride) {
  const int t = blockIdx.x;
  const int g_kv = blockIdx.y;
  const int chunk = blockIdx.z;
  const int nmem = min(tile_nmembers[t], SP_TILE_ROWS / gqa);
  if (nmem <= 0 || chunk >= tile_chunks[t] || chunk >= max_chunks) return;
  // the chunk must lie inside the block table (metadata is host-built; a
  // bad table must not become an out-of-bounds read)
  if ((int64_t)(chunk + 1) * ATTN_DECODE_CHUNK > (int64_t)max_blocks * block_size) return;
  const int* trow = tile_rows + (int64_t)t * SP_TILE_ROWS;
  const int b0 = trow[0];
  if (b0 < 0 || b0 >= B) return;
  const int nrows = nmem * gqa;
  const int nrb = (nrows + 31) >> 5;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int half = lane >> 5;
  const int col = lane & 31;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;                                                    // [128][256B] swizzled
  short* vt_lds = reinterpret_cast<short*>(smem + SP_ROUND_KEYS * ATTN_K_ROW_BYTES);  // [128][136]
  float* o_lds = reinterpret_cast<float*>(smem);                         // [4][32][132] (epilogue)
  float* ml_lds = reinterpret_cast<float*>(
      smem + (SP_STAGE_BYTES > SP_MERGE_BYTES ? SP_STAGE_BYTES : SP_MERGE_BYTES));  // [4][32][2]

  // this lane's query row in each 32-row block (B-operand column)
  const bf16_t* q_ptr[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int R = rb * 32 + col;
    const int mem = R / gqa;
    int brow = (R < nrows) ? trow[mem] : -1;
    if (brow >= B) brow = -1;
    q_ptr[rb] = (brow >= 0)
        ? q + (int64_t)brow * q_tstride + (g_kv * gqa + (R - mem * gqa)) * 128
        : nullptr;
  }

  f32x16 o_acc[2][4] = {};
  float m_run[2] = {-INFINITY, -INFINITY};
  float l_run[2] = {0.0f, 0.0f};

  const int* bt = block_tables + (int64_t)b0 * max_blocks;
  const int key_base = chunk * ATTN_DECODE_CHUNK;

#pragma unroll 1   // the two rounds stay a loop: one copy of the round body
  for (int round = 0; round < ATTN_DECODE_CHUNK / SP_ROUND_KEYS; ++round) {
    // ---- stage K (swizzled) + V^T: 128 keys x 8 slivers of 16 dims ---------
#pragma unroll
    for (int it = 0; it < SP_ROUND_KEYS * 8 / SP_THREADS; ++it) {
      const int slot = it * SP_THREADS + tid;
      const int key = slot >> 3;
      const int piece = slot & 7;
      const int gk = key_base + round * SP_ROUND_KEYS + key;
      int blk = bt[gk / block_size];
      blk = min(max(blk, 0), num_blocks - 1);
      const int64_t row = ((int64_t)blk * num_kv_heads + g_kv) * block_size + (gk % block_size);
      bf16x8_vec ka, kb, va, vb;
      if constexpr (FP8) {
        const u8x16_vec k8 = *reinterpret_cast<const u8x16_vec*>(k_cache + row * 128 + piece * 16);
        const u8x16_vec v8 = *reinterpret_cast<const u8x16_vec*>(v_cache + row * 128 + piece * 16);
        const float ks = k_scale[row];
        const float vs = v_scale[row];
        dequant_sliver(k8, ks, v8, vs, ka, kb, va, vb);
      } else {
        const bf16x8_vec* kp = reinterpret_cast<const bf16x8_vec*>(k_cache + row * 256) + piece * 2;
        const bf16x8_vec* vp = reinterpret_cast<const bf16x8_vec*>(v_cache + row * 256) + piece * 2;
        ka = kp[0]; kb = kp[1];
        va = vp[0]; vb = vp[1];
      }
      stage_sliver<SP_VT_ROW>(k_lds, vt_lds, key, piece, ka, kb, va, vb);
    }
    __syncthreads();

    // ---- this wave's 32 keys against each 32-row block ---------------------
    const int krow = wave * 32 + col;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      if (rb < nrb) {
        // Q re-read per round (L2-resident, 2 rounds) so it does not pin 64
        // VGPRs
        const f32x16 s_acc = qk_subtile(k_lds, krow, half, [&](int s) {
          bf16x8_mfma qf = {};
          if (q_ptr[rb] != nullptr)
            qf = *reinterpret_cast<const bf16x8_mfma*>((const short*)q_ptr[rb] + s * 16 + half * 8);
          return qf;
        });

        float sv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) sv[r] = s_acc[r] * scale;

        softmax_pv_subtile<SP_VT_ROW, false, false>(sv, m_run[rb], l_run[rb], o_acc[rb], vt_lds,
                                                    wave * 32, col, half);
      }
    }
    __syncthreads();   // staging buffers are rewritten next round / by the merge
  }

  // ---- merge the four key-split waves per 32-row block, write partials -----
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    if (rb < nrb) {
      const float l_row = half_merge_sum(l_run[rb]);
      float* ow = o_lds + ((wave * 32 + col) * SP_O_STRIDE);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g2 = 0; g2 < 4; ++g2) store_o_f32(ow, o_acc[rb][dt], dt, g2, half);
      if (half == 0) {
        ml_lds[(wave * 32 + col) * 2] = m_run[rb];
        ml_lds[(wave * 32 + col) * 2 + 1] = l_row;
      }
      __syncthreads();

      const int d2 = (tid & 63) * 2;
      for (int r = tid >> 6; r < 32; r += 4) {
        const int R = rb * 32 + r;
        if (R >= nrows) break;
        const int mem = R / gqa;
        const int brow = trow[mem];
        if (brow < 0 || brow >= B) continue;
        float mw[4];
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          mw[w] = ml_lds[(w * 32 + r) * 2];
          M = fmaxf(M, mw[w]);
        }
        float l_tot = 0.0f, a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const float wgt = __expf(mw[w] - M);
          l_tot += ml_lds[(w * 32 + r) * 2 + 1] * wgt;
          const float* orow = o_lds + (w * 32 + r) * SP_O_STRIDE + d2;
          a0 += orow[0] * wgt;
          a1 += orow[1] * wgt;
        }
        float* pg = partials +
            ((((int64_t)brow * num_kv_heads + g_kv) * max_chunks + chunk) * gqa + (R - mem * gqa)) *
                SP_PART_STRIDE;
        pg[d2] = a0;
        pg[d2 + 1] = a1;
        if (d2 == 0) {
          pg[128] = M;
          pg[129] = l_tot;
        }
      }
      __syncthreads();   // o_lds / ml_lds are reused by the next row block
    }
  }
}

// host-side launcher; n_tiles == 0 is the caller's to skip (no zero grids)
extern "C" void launch_attn_decode_shared(
    float* partials, const bf16_t* q, const void* k_cache, const void* v_cache,
    const float* k_scale, const float* v_scale, const int* block_tables,
    const int* tile_rows, const int* tile_nmembers, const int* tile_chunks,
    float scale, int B, int num_q_heads, int num_kv_heads, int num_blocks,
    int block_size, int max_blocks, int max_chunks, int q_tstride, int n_tiles,
    int cache_fp8, hipStream_t stream) {
  if (n_tiles <= 0 || max_chunks <= 0) return;
  const int gqa = num_q_heads / num_kv_heads;
  const dim3 grid(n_tiles, num_kv_heads, max_chunks);
  // > 64 KB of dynamic LDS needs the opt-in attribute (once per kernel and
  // device)
  static bool attr_set[2][64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  dev = (dev >= 0 && dev < 64) ? dev : 0;
#define SP_LAUNCH(F)                                                                       \
  do {                                                                                     \
    if (!attr_set[F ? 1 : 0][dev]) {                                                       \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_decode_shared_t<F>),   \
                                hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS_BYTES); \
      attr_set[F ? 1 : 0][dev] = true;                                                     \
    }                                                                                      \
    hipLaunchKernelGGL((attn_decode_shared_t<F>), grid, dim3(SP_THREADS), SP_LDS_BYTES,    \
                       stream, partials, q, (const char*)k_cache, (const char*)v_cache,    \
                       k_scale, v_scale, block_tables, tile_rows, tile_nmembers,           \
                       tile_chunks, scale, B, gqa, num_kv_heads, num_blocks, block_size,   \
                       max_blocks, max_chunks, q_tstride);                                 \
  } while (0)
  if (cache_fp8) SP_LAUNCH(true); else SP_LAUNCH(false);
#undef SP_LAUNCH
}
