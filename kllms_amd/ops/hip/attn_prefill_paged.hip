// Paged ("append" / "extend") causal prefill attention for gfx950 — the flash
// MFMA tile core of attn_mfma.h with its K/V tiles gathered from the paged
// cache.
//
// Sequence s has q_start[s] keys already in the cache and q_len[s] =
// cu_q[s+1] - cu_q[s] new tokens packed at rows cu_q[s].. of q/out. Row i of
// the sequence attends to keys 0 .. q_start[s] + i inclusive, ALL read from
// k_cache / v_cache through block_tables[s] (one table row per sequence):
// store_kv has written the new tokens' K/V before attention runs, so there
// are no k / v arguments. bf16 or e4m3 caches; e4m3 rows are dequantised as
// bf16(fp8 * row_scale) on the way into LDS.
//
// Structure (see attn_mfma.h for the fragment maps and the LDS layouts):
//   - an 8-wave workgroup serves up to 8 32-row q-tiles of ONE (sequence,
//     q-head); the waves share the K/V staging. How many tiles the host packs
//     per workgroup is its choice (grp_qpos0 = -1 marks an idle wave, which
//     still helps staging): few tiles per workgroup give a short chunk more
//     workgroups;
//   - 64 keys per barrier round; the NEXT round's global loads are issued
//     before this round's MFMA work and written to LDS after it, so the
//     gather latency overlaps the compute;
//   - a 32-key sub-tile lying wholly at or below the wave's first row limit
//     (all prefix keys, and the new keys of earlier tiles) takes no mask; only
//     sub-tiles overlapping the wave's own diagonal are masked.
//
// Robustness: the sequence index, block ids and table indices are clamped,
// the key loop never passes max_blocks * block_size, rows past q_len are
// never stored.
//
// Key splits (SP = PPSplit): a workgroup also gets a key range
// [kbeg, kend), kbeg a multiple of 64, and walks only the rounds inside it. A
// workgroup of a split sequence (grp_split >= 0) does not normalise: per
// (row, head, split) it writes the fp32 unnormalised O[128] and (m, l) — its
// softmax reference and the sum of p relative to it — to a workspace slot
// (seq_ws_base[s] + row * seq_nsplit[s] + split), and attn_prefill_paged_reduce
// merges a row's slots in split order. A row that sees no key of the range
// writes (m, l, O) = (-inf, 0, 0). Workgroups with grp_split = -1 keep the
// direct epilogue, so one launch serves split and unsplit sequences. kbeg,
// kend, the split index and the slot are clamped like the rest.

#include "attn_mfma.h"
#include "launch.h"

typedef float pp_f32x2 __attribute__((ext_vector_type(2)));

#define PP_QBLK 32
#define PP_KVBLK 64                // staged keys per barrier round (2 MFMA sub-tiles)
#define PP_NWAVES 8
#define PP_VT_ROW 72               // shorts: 64 keys + 8 pad (conflict-free b128 reads)

// one thread's share of a staged round: a 16-dim sliver of one key's K and V
template <bool FP8> struct PPRegs;
template <> struct PPRegs<false> { bf16x8_vec ka, kb, va, vb; };
template <> struct PPRegs<true> { u8x16_vec k8, v8; float ks, vs; };

// split-mode arguments: the plan's per-workgroup and per-sequence tensors and
// the partial workspace
struct PPSplit {
  static constexpr bool enabled = true;
  const int* grp_krange;     // [G * 2]: kbeg, kend
  const int* grp_split;      // [G]: split index, -1 = direct epilogue
  const int* seq_nsplit;     // [n_seq]
  const int* seq_ws_base;    // [n_seq]: first workspace slot of the sequence
  float* part_o;             // [ws_rows, H, 128]
  float* part_ml;            // [ws_rows, H, 2]
  int ws_rows;
  int max_splits;
};

struct PPNoSplit { static constexpr bool enabled = false; };

// SP = PPNoSplit: the whole key range and the direct epilogue; the trailing
// argument is empty and every split branch is compiled out
template <bool FP8, typename SP = PPNoSplit>
__global__ __launch_bounds__(64 * PP_NWAVES) void attn_prefill_paged_t(
    bf16_t* __restrict__ out,            // [T, H, 128] contiguous
    const bf16_t* __restrict__ q,        // [T, H, 128], token stride q_tstride
    const char* __restrict__ k_cache,    // [NB, KVH, BS, 128], bf16 or fp8
    const char* __restrict__ v_cache,
    const float* __restrict__ k_scale,   // [NB, KVH, BS] per-row dequant (FP8 only)
    const float* __restrict__ v_scale,
    const int* __restrict__ block_tables,   // [n_seq, max_blocks]
    const int* __restrict__ cu_q,           // [n_seq + 1]
    const int* __restrict__ q_start,        // [n_seq]
    const int* __restrict__ grp_seq,        // [G]
    const int* __restrict__ grp_qpos0,      // [G * 8], -1 = idle wave
    float scale, int n_seq, int total_rows, int num_q_heads, int num_kv_heads,
    int num_blocks, int block_size, int max_blocks, int q_tstride, SP sp) {
  constexpr bool SPLIT = SP::enabled;
  const int grp = blockIdx.x;
  const int h = blockIdx.y;
  const int g_kv = h / (num_q_heads / num_kv_heads);
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int half = lane >> 5;
  const int col = lane & 31;       // q-row (B/C col) or K/VT row (A row)

  const int seq = min(max(grp_seq[grp], 0), n_seq - 1);
  const int row0 = cu_q[seq];
  const int qlen = min(cu_q[seq + 1], total_rows) - row0;
  if (row0 < 0 || qlen <= 0) return;             // workgroup-uniform
  const int start = max(q_start[seq], 0);
  const int qpos0 = grp_qpos0[grp * PP_NWAVES + wave];   // -1: idle wave
  const bool active = qpos0 >= 0 && qpos0 < qlen;
  const int my_qpos = active ? qpos0 + col : 0;
  const int my_limit = start + my_qpos;          // last key this row sees
  const int kv_cap = (int)min((int64_t)max_blocks * block_size, (int64_t)0x7fffffff);

  __shared__ __attribute__((aligned(16))) char smem[PP_KVBLK * ATTN_K_ROW_BYTES +
                                                    128 * PP_VT_ROW * 2];
  char* k_lds = smem;                                   // [64][256B], XOR-swizzled
  short* vt_lds = reinterpret_cast<short*>(smem + PP_KVBLK * ATTN_K_ROW_BYTES);  // [128][72]

  // ---- Q fragments (B-operand): 8 d-slices of 16 --------------------------
  bf16x8_mfma q_frag[8];
  {
    const int qrow_c = row0 + (active ? min(my_qpos, qlen - 1) : 0);
    const bf16_t* qp = q + (int64_t)qrow_c * q_tstride + h * 128;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      q_frag[s] = *reinterpret_cast<const bf16x8_mfma*>((const short*)qp + s * 16 + half * 8);
  }

  f32x16 o_acc[4] = {};
  float m_run = -INFINITY;
  float l_run = 0.0f;

  // workgroup-wide kv bound: the furthest key any active wave may see
  int kv_end_grp = 0;
#pragma unroll
  for (int w = 0; w < PP_NWAVES; ++w) {
    const int qp0 = grp_qpos0[grp * PP_NWAVES + w];
    if (qp0 >= 0 && qp0 < qlen) kv_end_grp = max(kv_end_grp, start + min(qlen, qp0 + PP_QBLK));
  }
  kv_end_grp = min(kv_end_grp, kv_cap);
  int kv_end_me = active ? min(start + min(qlen, qpos0 + PP_QBLK), kv_cap) : 0;
  int kbeg = 0;
  if constexpr (SPLIT) {
    // the workgroup's key range, cut to the causal bound
    const int kend = max(sp.grp_krange[grp * 2 + 1], 0);
    kbeg = min(max(sp.grp_krange[grp * 2], 0), kv_cap) & ~(PP_KVBLK - 1);
    kv_end_grp = min(kv_end_grp, kend);
    kv_end_me = min(kv_end_me, kend);
  }

  const int* bt = block_tables + (int64_t)seq * max_blocks;
  const int st_key = tid >> 3;               // one key per 8 threads
  const int st_piece = tid & 7;              // 16-dim sliver of that key

  // global -> registers for the round starting at key kt00
  auto load_round = [&](int kt00, PPRegs<FP8>& r) {
    const int gk = kt00 + st_key;
    if (gk < kv_end_grp) {
      int blk = bt[min(gk / block_size, max_blocks - 1)];
      blk = min(max(blk, 0), num_blocks - 1);
      const int64_t row = ((int64_t)blk * num_kv_heads + g_kv) * block_size + (gk % block_size);
      if constexpr (FP8) {
        r.k8 = *reinterpret_cast<const u8x16_vec*>(k_cache + row * 128 + st_piece * 16);
        r.v8 = *reinterpret_cast<const u8x16_vec*>(v_cache + row * 128 + st_piece * 16);
        r.ks = k_scale[row];
        r.vs = v_scale[row];
      } else {
        const bf16x8_vec* kp = reinterpret_cast<const bf16x8_vec*>(k_cache + row * 256) + st_piece * 2;
        const bf16x8_vec* vp = reinterpret_cast<const bf16x8_vec*>(v_cache + row * 256) + st_piece * 2;
        r.ka = kp[0]; r.kb = kp[1];
        r.va = vp[0]; r.vb = vp[1];
      }
    } else {                                  // past the bound: zero rows
      if constexpr (FP8) {
        r.k8 = u8x16_vec{}; r.v8 = u8x16_vec{}; r.ks = 0.0f; r.vs = 0.0f;
      } else {
        r.ka = bf16x8_vec{}; r.kb = bf16x8_vec{}; r.va = bf16x8_vec{}; r.vb = bf16x8_vec{};
      }
    }
  };

  // registers -> LDS: K swizzled, V transposed
  auto store_round = [&](const PPRegs<FP8>& r) {
    bf16x8_vec ka, kb, va, vb;
    if constexpr (FP8) {
      dequant_sliver(r.k8, r.ks, r.v8, r.vs, ka, kb, va, vb);
    } else {
      ka = r.ka; kb = r.kb; va = r.va; vb = r.vb;
    }
    stage_sliver<PP_VT_ROW>(k_lds, vt_lds, st_key, st_piece, ka, kb, va, vb);
  };

  PPRegs<FP8> regs;
  load_round(kbeg, regs);

  for (int kt00 = kbeg; kt00 < kv_end_grp; kt00 += PP_KVBLK) {
    const int nkeys_blk = min(PP_KVBLK, kv_end_grp - kt00);
    store_round(regs);
    __syncthreads();
    // next round's gather flies under this round's MFMA work
    if (kt00 + PP_KVBLK < kv_end_grp) load_round(kt00 + PP_KVBLK, regs);

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
    const int kt0 = kt00 + sub * 32;
    const int nkeys = min(32, nkeys_blk - sub * 32);
    if (active && kt0 < kv_end_me && nkeys > 0) {
      const f32x16 s_acc = qk_subtile(k_lds, col + sub * 32, half,
                                      [&](int s) { return q_frag[s]; });

      // ---- scale (+ causal mask on the diagonal sub-tiles only) ------------
      // every key of a sub-tile ending at or before the wave's FIRST row limit
      // is visible to all 32 rows (and is below kv_end_grp, so it is staged)
      float sv[16];
      if (nkeys == 32 && kt0 + 31 <= start + qpos0) {        // wave-uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) sv[r] = s_acc[r] * scale;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = acc_row(r, half);
          const bool ok = (kt0 + kr <= my_limit) && (kr < nkeys);
          sv[r] = ok ? s_acc[r] * scale : -INFINITY;
        }
      }

      // a row that has seen no key yet and sees none here (a split range above
      // its causal limit) keeps m_run = -inf and adds p = 0
      softmax_pv_subtile<PP_VT_ROW, true, true>(sv, m_run, l_run, o_acc, vt_lds, sub * 32,
                                                col, half);
    }
    }  // sub
    __syncthreads();   // the staging buffers are rewritten next round
  }

  // ---- epilogue: merge half-sums, normalize, write O ----------------------
  l_run = half_merge_sum(l_run);
  if constexpr (SPLIT) {
    const int split = sp.grp_split[grp];            // workgroup-uniform
    if (split >= 0) {
      // partial of (row, head, split): unnormalised O, reference m, sum l. A
      // wave whose loop never ran writes (-inf, 0, 0) from its initial state.
      if (active && my_qpos < qlen) {
        const int nsplit = min(max(sp.seq_nsplit[seq], 1), sp.max_splits);
        int64_t slot = (int64_t)sp.seq_ws_base[seq] + (int64_t)my_qpos * nsplit +
                       min(split, nsplit - 1);
        slot = min(max(slot, (int64_t)0), (int64_t)sp.ws_rows - 1);
        const int64_t cell = slot * num_q_heads + h;
        float* po = sp.part_o + cell * 128;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int g2 = 0; g2 < 4; ++g2) store_o_f32(po, o_acc[dt], dt, g2, half);
        if (half == 0) {
          pp_f32x2 ml;
          ml[0] = m_run;
          ml[1] = l_run;
          *reinterpret_cast<pp_f32x2*>(sp.part_ml + cell * 2) = ml;
        }
      }
      return;
    }
  }
  if (active && my_qpos < qlen) {
    const float inv_l = (l_run > 0.0f) ? 1.0f / l_run : 0.0f;
    bf16_t* op = out + (((int64_t)(row0 + my_qpos)) * num_q_heads + h) * 128;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g2 = 0; g2 < 4; ++g2) store_o_bf16(op, o_acc[dt], inv_l, dt, g2, half);
  }
}

// Merge of the split partials: block (t, 8-head group), 32 threads per head,
// 4 dims per thread. With j over the row's splits in index order and
// w_j = exp(m_j - max_j m_j) (0 for an empty partial: l_j = 0 or m_j = -inf),
// out = sum_j w_j O_j / sum_j w_j l_j, zeros when the denominator is 0. The
// order is fixed, so the result does not depend on which workgroup finished
// first. Rows of unsplit sequences are left alone.
#define PP_RED_HEADS 8
__global__ __launch_bounds__(32 * PP_RED_HEADS) void attn_prefill_paged_reduce(
    bf16_t* __restrict__ out, const float* __restrict__ part_o,
    const float* __restrict__ part_ml, const int* __restrict__ cu_q,
    const int* __restrict__ seq_nsplit, const int* __restrict__ seq_ws_base,
    int n_seq, int total_rows, int num_q_heads, int ws_rows, int max_splits) {
  const int t = blockIdx.x;
  const int h = blockIdx.y * PP_RED_HEADS + (threadIdx.x >> 5);
  const int d0 = (threadIdx.x & 31) * 4;
  if (t >= total_rows || h >= num_q_heads) return;
  // the sequence holding packed row t: last s with cu_q[s] <= t
  int lo = 0, hi = n_seq - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cu_q[mid] <= t) lo = mid; else hi = mid - 1;
  }
  const int seq = lo;
  const int row = t - cu_q[seq];
  const int nsplit = min(seq_nsplit[seq], max_splits);
  if (nsplit < 2 || row < 0 || t >= cu_q[seq + 1]) return;
  const int64_t slot0 = (int64_t)seq_ws_base[seq] + (int64_t)row * nsplit;
  auto cell_of = [&](int j) {
    const int64_t slot = min(max(slot0 + j, (int64_t)0), (int64_t)ws_rows - 1);
    return slot * num_q_heads + h;
  };
  float m_all = -INFINITY;
  for (int j = 0; j < nsplit; ++j) {
    const pp_f32x2 ml = *reinterpret_cast<const pp_f32x2*>(part_ml + cell_of(j) * 2);
    if (ml[1] > 0.0f) m_all = fmaxf(m_all, ml[0]);
  }
  f32x4 acc = {};
  float den = 0.0f;
  for (int j = 0; j < nsplit; ++j) {
    const int64_t cell = cell_of(j);
    const pp_f32x2 ml = *reinterpret_cast<const pp_f32x2*>(part_ml + cell * 2);
    if (!(ml[1] > 0.0f) || ml[0] == -INFINITY) continue;     // empty partial
    const float w = __expf(ml[0] - m_all);
    const f32x4 o = *reinterpret_cast<const f32x4*>(part_o + cell * 128 + d0);
    den += w * ml[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += w * o[i];
  }
  const float inv = (den > 0.0f) ? 1.0f / den : 0.0f;
  uint64_t word = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    word |= ((uint64_t)(uint16_t)f32_to_bf16(acc[i] * inv)) << (16 * i);
  *reinterpret_cast<uint64_t*>((short*)(out + ((int64_t)t * num_q_heads + h) * 128) + d0) = word;
}

// the one launch of attn_prefill_paged_t, behind both entry points
template <bool FP8, typename SP>
static void pp_launch(
    bf16_t* out, const bf16_t* q, const void* k_cache, const void* v_cache,
    const float* k_scale, const float* v_scale, const int* block_tables,
    const int* cu_q, const int* q_start, const int* grp_seq, const int* grp_qpos0,
    float scale, int n_seq, int total_rows, int num_q_heads, int num_kv_heads,
    int num_blocks, int block_size, int max_blocks, int q_tstride, int n_groups,
    SP sp, hipStream_t stream) {
  hipLaunchKernelGGL((attn_prefill_paged_t<FP8, SP>), dim3(n_groups, num_q_heads),
                     dim3(64 * PP_NWAVES), 0, stream,
                     out, q, (const char*)k_cache, (const char*)v_cache, k_scale, v_scale,
                     block_tables, cu_q, q_start, grp_seq, grp_qpos0, scale, n_seq,
                     total_rows, num_q_heads, num_kv_heads, num_blocks, block_size,
                     max_blocks, q_tstride, sp);
}

// host-side launcher; an empty grid is the caller's to skip
extern "C" void launch_attn_prefill_paged(
    bf16_t* out, const bf16_t* q, const void* k_cache, const void* v_cache,
    const float* k_scale, const float* v_scale, const int* block_tables,
    const int* cu_q, const int* q_start, const int* grp_seq, const int* grp_qpos0,
    float scale, int n_seq, int total_rows, int num_q_heads, int num_kv_heads,
    int num_blocks, int block_size, int max_blocks, int q_tstride, int n_groups,
    int cache_fp8, hipStream_t stream) {
  if (n_groups <= 0 || n_seq <= 0 || total_rows <= 0) return;
  (cache_fp8 ? pp_launch<true, PPNoSplit> : pp_launch<false, PPNoSplit>)(
      out, q, k_cache, v_cache, k_scale, v_scale, block_tables, cu_q, q_start, grp_seq,
      grp_qpos0, scale, n_seq, total_rows, num_q_heads, num_kv_heads, num_blocks, block_size,
      max_blocks, q_tstride, n_groups, PPNoSplit{}, stream);
}

// split launch + merge; the caller has checked the workspace against ws_rows
extern "C" void launch_attn_prefill_paged_split(
    bf16_t* out, const bf16_t* q, const void* k_cache, const void* v_cache,
    const float* k_scale, const float* v_scale, const int* block_tables,
    const int* cu_q, const int* q_start, const int* grp_seq, const int* grp_qpos0,
    const int* grp_krange, const int* grp_split, const int* seq_nsplit,
    const int* seq_ws_base, float* part_o, float* part_ml, int ws_rows, int max_splits,
    float scale, int n_seq, int total_rows, int num_q_heads, int num_kv_heads,
    int num_blocks, int block_size, int max_blocks, int q_tstride, int n_groups,
    int cache_fp8, hipStream_t stream) {
  if (n_groups <= 0 || n_seq <= 0 || total_rows <= 0 || ws_rows <= 0) return;
  const PPSplit sp{grp_krange, grp_split, seq_nsplit, seq_ws_base, part_o, part_ml,
                   ws_rows, max_splits};
  (cache_fp8 ? pp_launch<true, PPSplit> : pp_launch<false, PPSplit>)(
      out, q, k_cache, v_cache, k_scale, v_scale, block_tables, cu_q, q_start, grp_seq,
      grp_qpos0, scale, n_seq, total_rows, num_q_heads, num_kv_heads, num_blocks, block_size,
      max_blocks, q_tstride, n_groups, sp, stream);
  const dim3 rgrid(total_rows, (num_q_heads + PP_RED_HEADS - 1) / PP_RED_HEADS);
  hipLaunchKernelGGL(attn_prefill_paged_reduce, rgrid, dim3(32 * PP_RED_HEADS), 0, stream,
                     out, part_o, part_ml, cu_q, seq_nsplit, seq_ws_base, n_seq, total_rows,
                     num_q_heads, ws_rows, max_splits);
}
