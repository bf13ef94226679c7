// The bf16 MFMA flash-attention tile core shared by attn_prefill.hip,
// attn_prefill_paged.hip and attn_decode_shared.hip (head_dim 128).
//
// One wave owns 32 query rows and walks the keys in 32-key sub-tiles of a
// round that the whole workgroup staged in LDS:
//   - K rows of 256 bytes, XOR-swizzled (G4: row-major tiles at D=128 are an
//     up-to-16-way ds_read_b128 conflict; byte ^= (row&15)<<4 makes the
//     16-lane group conflict-free); V staged TRANSPOSED ([128][keys + 8 pad])
//     so the PV A-fragment reads are contiguous 16B;
//   - SWAPPED QK^T: S = mfma(A=K_tile, B=Q) so each lane's accumulators hold
//     one q-row's scores -> softmax is in-register (fmax chain + one
//     permlane32_swap half-merge), no cross-lane LDS traffic;
//   - P repacked to bf16 MFMA B-fragments with pack + permlane32_swap half
//     exchanges (T12/T21 pattern);
//   - PV as O^T = mfma(A=V^T, B=P) over 4 d-tiles;
//   - online softmax with per-lane running max/sum (rows are lane-local; the
//     two half-waves of a row hold 16 keys each, so l_run is a half-sum until
//     half_merge_sum in the epilogue).
//
// MFMA fragment maps (v_mfma_f32_32x32x16_bf16, verified on-device by the
// mfma_selftest binding):
//   A[i][k]: lane l holds i = l&31, k = (l>>5)*8 + j   (j = 0..7)
//   B[k][j]: lane l holds j = l&31, k = (l>>5)*8 + jj
//   C/D[i][j]: lane l holds j = l&31, i = (r&3) + 8*(r>>2) + 4*(l>>5)  (r = 0..15)
// Throughout, half = lane >> 5 and col = lane & 31 (q-row as B/C column, K /
// V^T row as A row).
//
// Masking, the softmax scale and all global addressing stay with the kernels.
#pragma once

#include "common.h"

typedef __bf16 bf16x8_mfma __attribute__((ext_vector_type(8)));

#define ATTN_K_ROW_BYTES 256       // one staged K row: 128 bf16
#define ATTN_DEFER_THR 8.0f        // defer-max: P stays below e^8

__device__ __forceinline__ int acc_row(int r, int half) {
  return (r & 3) + 8 * (r >> 2) + 4 * half;   // C/D row map
}

// a row's two half-waves hold disjoint keys: merge their max / sum
__device__ __forceinline__ float half_merge_max(float x) {
  auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}

__device__ __forceinline__ float half_merge_sum(float x) {
  auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

// One thread's share of a staged round, registers -> LDS: the 16-dim sliver
// `piece` of row `key` of the round, K swizzled, V transposed ([128][VT_ROW]).
template <int VT_ROW>
__device__ __forceinline__ void stage_sliver(char* k_lds, short* vt_lds, int key, int piece,
                                             bf16x8_vec ka, bf16x8_vec kb,
                                             bf16x8_vec va, bf16x8_vec vb) {
  const int swz = (key & 15) << 4;
  *reinterpret_cast<bf16x8_vec*>(k_lds + key * ATTN_K_ROW_BYTES + ((piece * 32) ^ swz)) = ka;
  *reinterpret_cast<bf16x8_vec*>(k_lds + key * ATTN_K_ROW_BYTES + ((piece * 32 + 16) ^ swz)) = kb;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    vt_lds[(piece * 16 + j) * VT_ROW + key] = va[j];
    vt_lds[(piece * 16 + 8 + j) * VT_ROW + key] = vb[j];
  }
}

// One thread's e4m3 sliver, 16 bytes of a K row and 16 of a V row with their
// row scales -> bf16(fp8 * row_scale)
__device__ __forceinline__ void dequant_sliver(u8x16_vec k8, float ks, u8x16_vec v8, float vs,
                                               bf16x8_vec& ka, bf16x8_vec& kb,
                                               bf16x8_vec& va, bf16x8_vec& vb) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ka[j] = f32_to_bf16(fp8_to_f32(k8[j]) * ks);
    kb[j] = f32_to_bf16(fp8_to_f32(k8[8 + j]) * ks);
    va[j] = f32_to_bf16(fp8_to_f32(v8[j]) * vs);
    vb[j] = f32_to_bf16(fp8_to_f32(v8[8 + j]) * vs);
  }
}

// QK^T (swapped) of the 32 staged keys whose row this lane reads as `krow`:
// S[key][qrow] over 8 d-slices, unscaled. q_frag(s) gives the lane's B
// fragment of d-slice s: dims s*16 + half*8 .. +7 of its q-row, from
// registers or, where 8 resident fragments would cost too many, loaded here.
template <typename QFrag>
__device__ __forceinline__ f32x16 qk_subtile(const char* k_lds, int krow, int half,
                                             QFrag q_frag) {
  f32x16 s_acc = {};
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const bf16x8_mfma qf = q_frag(s);
    const int byte_off = (s * 2 + half) * 16;
    const bf16x8_mfma a_frag = *reinterpret_cast<const bf16x8_mfma*>(
        k_lds + krow * ATTN_K_ROW_BYTES + (byte_off ^ ((krow & 15) << 4)));
    s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_frag, qf, s_acc, 0, 0, 0);
  }
  return s_acc;
}

// Online-softmax step and O^T += V^T x P for one 32-key sub-tile whose keys
// start at column key_off of the staged V^T. sv holds the lane's 16 scaled
// (and, if MASKED, -inf masked) scores.
//   DEFER_MAX (T13): rows are lane-local, so the decision is per-lane — keep
//     the old running max while the tile max grew < ATTN_DEFER_THR (P then
//     bounded by e^THR, fine for f32 p / bf16 pack), decided BEFORE this
//     tile's P is exponentiated (the safe order), and skip the rescale when
//     no lane needs it. A first tile (m_run = -inf) never defers; a row that
//     has seen no key and sees none here has tmax = m_run = -inf, keeps m_run
//     and adds p = 0. Off: always take the new max and rescale.
//   MASKED: scores may be -inf and then give p = 0 (also when m_new = -inf).
template <int VT_ROW, bool DEFER_MAX, bool MASKED>
__device__ __forceinline__ void softmax_pv_subtile(const float (&sv)[16], float& m_run,
                                                   float& l_run, f32x16 (&o_acc)[4],
                                                   const short* vt_lds, int key_off,
                                                   int col, int half) {
  float tmax = sv[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, sv[r]);
  tmax = half_merge_max(tmax);

  float m_new, alpha;
  if (DEFER_MAX && tmax <= m_run + ATTN_DEFER_THR) {
    m_new = m_run;
    alpha = 1.0f;
  } else {
    m_new = fmaxf(m_run, tmax);
    alpha = (m_run == -INFINITY) ? 0.0f : __expf(m_run - m_new);
  }
  m_run = m_new;
  if (!DEFER_MAX || __builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o_acc[dt][r] *= alpha;
  }

  float p[16];
  float psum = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    p[r] = (MASKED && sv[r] == -INFINITY) ? 0.0f : __expf(sv[r] - m_new);
    psum += p[r];
  }
  l_run = l_run * alpha + psum;

  // repack P -> bf16 B-fragments (T12/T21 half swaps)
  uint32_t packs[8];
#pragma unroll
  for (int pr = 0; pr < 8; ++pr) {
    const short lo = f32_to_bf16(p[2 * pr]);
    const short hi = f32_to_bf16(p[2 * pr + 1]);
    packs[pr] = ((uint32_t)(uint16_t)hi << 16) | (uint16_t)lo;
  }
  uint32_t bfrag[2][4];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    auto r0 = __builtin_amdgcn_permlane32_swap(packs[4 * kt + 0], packs[4 * kt + 2], false, false);
    auto r1 = __builtin_amdgcn_permlane32_swap(packs[4 * kt + 1], packs[4 * kt + 3], false, false);
    bfrag[kt][0] = r0[0];
    bfrag[kt][1] = r1[0];
    bfrag[kt][2] = r0[1];
    bfrag[kt][3] = r1[1];
  }

  // PV: O^T += V^T x P over 4 d-tiles
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const int d_row = dt * 32 + col;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const bf16x8_mfma vfrag = *reinterpret_cast<const bf16x8_mfma*>(
          vt_lds + d_row * VT_ROW + key_off + kt * 16 + half * 8);
      bf16x8_mfma pfrag;
      {
        uint32_t* pf = reinterpret_cast<uint32_t*>(&pfrag);
#pragma unroll
        for (int w = 0; w < 4; ++w) pf[w] = bfrag[kt][w];
      }
      o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag, pfrag, o_acc[dt], 0, 0, 0);
    }
  }
}

// Epilogue stores of the lane's dims of d-tile dt: accumulator registers
// 4*g2..+3 are the 4 consecutive dims from dt*32 + 8*g2 + 4*half.
// Normalised bf16, one 8-byte store; `row` is the q-row's 128 outputs.
__device__ __forceinline__ void store_o_bf16(bf16_t* row, const f32x16& o, float inv_l,
                                             int dt, int g2, int half) {
  const int d0 = dt * 32 + 8 * g2 + 4 * half;
  uint64_t word = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float val = o[4 * g2 + j] * inv_l;
    word |= ((uint64_t)(uint16_t)f32_to_bf16(val)) << (16 * j);
  }
  *reinterpret_cast<uint64_t*>((short*)row + d0) = word;
}

// Raw fp32, one 16-byte store
__device__ __forceinline__ void store_o_f32(float* row, const f32x16& o, int dt, int g2, int half) {
  const int d0 = dt * 32 + 8 * g2 + 4 * half;
  f32x4 v4;
#pragma unroll
  for (int j = 0; j < 4; ++j) v4[j] = o[4 * g2 + j];
  *reinterpret_cast<f32x4*>(row + d0) = v4;
}
