// Varlen causal prefill attention for gfx950 — flash-style MFMA kernel over
// packed, contiguous K/V. The tile core (LDS layouts, fragment maps, swapped
// QK^T, online softmax with defer-max, P repack, PV) is attn_mfma.h.
//
// Structure (cdna_hip_programming.md Appendix B "Fused attention prefill"):
//   - an 8-WAVE workgroup serves 8 consecutive 32-row q-tiles of ONE
//     (sequence, q-head): the K/V LDS staging is shared by the 8 waves, so
//     its cost is amortized 8x over the 1-wave-per-block version;
//   - 64 keys staged per barrier round, two 32-key sub-tiles per wave.
//
// Host metadata (built in ops/__init__._prefill_tiles): q-tiles grouped 4 per
// block PER SEQUENCE; grp_qpos0 = -1 pads idle waves.

#include "attn_mfma.h"
#include "launch.h"

#define QBLK 32
#define KVBLK 64                   // staged keys per barrier round (2 MFMA sub-tiles)
#define DHEAD 128
#define NWAVES 8
#define VT_ROW_SHORTS 72           // 64 keys + 8 pad (conflict-free b128 reads)

extern "C" __global__ void __launch_bounds__(64 * NWAVES) attn_prefill_kernel(
    bf16_t* __restrict__ out,       // [T, H, D] contiguous
    const bf16_t* __restrict__ q,   // [T, H, D], token stride q_tstride
    const bf16_t* __restrict__ k,   // [T, KVH, D], token stride kv_tstride
    const bf16_t* __restrict__ v,
    const int* __restrict__ grp_seq_start,   // [G] first token of the group's seq
    const int* __restrict__ grp_seqlen,      // [G]
    const int* __restrict__ grp_qpos0,       // [G*NWAVES], -1 = idle wave
    float scale, int num_q_heads, int num_kv_heads, int q_tstride, int kv_tstride) {
  const int grp = blockIdx.x;
  const int h = blockIdx.y;
  const int g_kv = h / (num_q_heads / num_kv_heads);
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int half = lane >> 5;
  const int col = lane & 31;       // q-row (B/C col) or K/VT row (A row)

  const int seq_start = grp_seq_start[grp];
  const int seqlen = grp_seqlen[grp];
  const int qpos0 = grp_qpos0[grp * NWAVES + wave];   // -1: idle wave
  const bool active = qpos0 >= 0;
  const int my_qpos = active ? qpos0 + col : 0;

  __shared__ __attribute__((aligned(16))) char smem[KVBLK * ATTN_K_ROW_BYTES +
                                                    DHEAD * VT_ROW_SHORTS * 2];
  char* k_lds = smem;                                   // [64][256B], XOR-swizzled
  short* vt_lds = reinterpret_cast<short*>(smem + KVBLK * ATTN_K_ROW_BYTES);  // [128][72]

  // ---- Q fragments (B-operand): 8 d-slices of 16 --------------------------
  bf16x8_mfma q_frag[8];
  {
    const int qrow_c = active ? min(my_qpos, seqlen - 1) : 0;
    const bf16_t* qp = q + (int64_t)(seq_start + qrow_c) * q_tstride + h * DHEAD;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      q_frag[s] = *reinterpret_cast<const bf16x8_mfma*>((const short*)qp + s * 16 + half * 8);
  }

  f32x16 o_acc[4] = {};
  float m_run = -INFINITY;
  float l_run = 0.0f;

  // group-wide kv bound: the group's last active wave reaches furthest
  int kv_end_grp = 0;
#pragma unroll
  for (int w = 0; w < NWAVES; ++w) {
    const int qp0 = grp_qpos0[grp * NWAVES + w];
    if (qp0 >= 0) kv_end_grp = max(kv_end_grp, min(seqlen, qp0 + QBLK));
  }
  const int kv_end_me = active ? min(seqlen, qpos0 + QBLK) : 0;

  for (int kt00 = 0; kt00 < kv_end_grp; kt00 += KVBLK) {
    const int nkeys_blk = min(KVBLK, kv_end_grp - kt00);

    // ---- stage K (swizzled) + V^T, all 512 threads cooperatively ----------
    {
      const int key = tid >> 3;               // one key per 8 threads
      const int piece = tid & 7;              // 16-dim sliver of that key
      const bool valid = key < nkeys_blk;     // rows past the bound are zeros
      const int64_t tok = seq_start + kt00 + min(key, nkeys_blk - 1);
      const bf16x8_vec* kp = reinterpret_cast<const bf16x8_vec*>(
          (const short*)(k + tok * kv_tstride + g_kv * DHEAD)) + piece * 2;
      const bf16x8_vec* vp = reinterpret_cast<const bf16x8_vec*>(
          (const short*)(v + tok * kv_tstride + g_kv * DHEAD)) + piece * 2;
      const bf16x8_vec zero = {0, 0, 0, 0, 0, 0, 0, 0};
      stage_sliver<VT_ROW_SHORTS>(k_lds, vt_lds, key, piece,
                                  valid ? kp[0] : zero, valid ? kp[1] : zero,
                                  valid ? vp[0] : zero, valid ? vp[1] : zero);
    }
    __syncthreads();

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int kt0 = kt00 + sub * 32;
      const int nkeys = min(32, nkeys_blk - sub * 32);
      if (active && kt0 < kv_end_me && nkeys > 0) {
        const f32x16 s_acc = qk_subtile(k_lds, col + sub * 32, half,
                                        [&](int s) { return q_frag[s]; });

        // ---- mask + scale --------------------------------------------------
        float sv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt0 + acc_row(r, half);
          const bool ok = (key <= my_qpos) && (acc_row(r, half) < nkeys) && (key < seqlen);
          sv[r] = ok ? s_acc[r] * scale : -INFINITY;
        }

        softmax_pv_subtile<VT_ROW_SHORTS, true, true>(sv, m_run, l_run, o_acc, vt_lds,
                                                      sub * 32, col, half);
      }
    }
    __syncthreads();
  }

  // ---- epilogue: merge half-sums, normalize, write O ----------------------
  l_run = half_merge_sum(l_run);
  if (active && my_qpos < seqlen) {
    const float inv_l = (l_run > 0.0f) ? 1.0f / l_run : 0.0f;
    bf16_t* op = out + (((int64_t)(seq_start + my_qpos)) * num_q_heads + h) * DHEAD;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g2 = 0; g2 < 4; ++g2) store_o_bf16(op, o_acc[dt], inv_l, dt, g2, half);
  }
}

extern "C" void launch_attn_prefill(bf16_t* out, const bf16_t* q, const bf16_t* k, const bf16_t* v,
                                    const int* grp_seq_start, const int* grp_seqlen,
                                    const int* grp_qpos0, float scale, int n_groups,
                                    int num_q_heads, int num_kv_heads, int q_tstride,
                                    int kv_tstride, hipStream_t stream) {
  hipLaunchKernelGGL(attn_prefill_kernel, dim3(n_groups, num_q_heads), dim3(64 * NWAVES), 0,
                     stream, out, q, k, v, grp_seq_start, grp_seqlen, grp_qpos0, scale,
                     num_q_heads, num_kv_heads, q_tstride, kv_tstride);
}
