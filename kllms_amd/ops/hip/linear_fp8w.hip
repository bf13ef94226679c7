// Weight-only fp8 (OCP e4m3) x bf16 GEMM for gfx950 (opt-in fp8 weights).
//
//   out[M, N] = bf16( (sum_k x[m, k] * q[n, k]) * scale[n] + bias[n] )
//
// x bf16 [M, K] (unit inner stride, row stride >= K), q e4m3 [N, K] K-contiguous,
// scale fp32 [N] per output channel, bias bf16 [N] or absent, 1 <= M <= 256,
// K % 64 == 0, N % 16 == 0.
//
// Numerics: e4m3 -> bf16 is exact (3 mantissa bits into 8), so the weight bytes
// are converted in registers and fed to v_mfma_f32_32x32x16_bf16 with EXACT
// products and fp32 accumulation; scale[n] and the bias touch only the fp32
// accumulator in the epilogue (a scale folded into a bf16-rounded weight would
// cost half a bf16 ulp per weight).
//
// Geometry: one block = 256 threads = 4 waves computes out[32*MT rows,
// 128 columns] over one K slice; wave w owns the 32 weight rows (output
// columns) [32w, 32w+32) and all 32*MT activation rows. The weight is the MFMA
// A operand (lane l: row n = l & 31), x the B operand (lane l: column
// m = l & 31), so D has n in the registers and m on the lane and each lane
// stores 4 consecutive n of one row m (8 B bf16 / 16 B fp32).
//
// Operand paths: the weights are streamed once and never shared between
// waves, so each lane loads 16-byte pieces of ITS row straight to VGPRs (no
// LDS round trip). One 16-byte piece holds two 8-deep MFMA k-steps; the
// order of k inside a 64-deep stage is therefore permuted (lane half h, piece
// p, step s <-> k = 32p + 16h + 8s + j) and the x fragment is read from LDS at
// that same k. x (<= 256 x K bf16, L2 resident, re-read by every column tile)
// is staged through LDS in full 128-byte lines (8 lanes per row), XOR-swizzled
// for conflict-free ds_read_b128, double-buffered with one barrier per stage.
// Both operands are prefetched three stages ahead in a register ring.
//
// Rows >= M and columns >= N are neither read nor written: out-of-range lanes
// load a clamped (valid) row and their results are dropped at the store.
//
// Split-K (small N cannot fill 256 CUs): each K slice writes an fp32 slab,
// a second launch sums the slabs in slice order and applies scale and bias.
// No atomics, no counters: the same call gives the same bits, and both
// launches are plain stream work (hipGraph-capturable).
//
// Batched form (the experts of a MoE layer): E such problems in one launch,
//   out[e, m, n] = bf16( (sum_k x_e[m, k] * q[e, n, k]) * scale[e, n] ),
// the same body per block with the expert index in the grid and per-expert
// offsets on x (0 = shared), q, scale, out and the slabs; no bias.

#include <algorithm>

#include "launch.h"

#define FW_BK 64                 // k per stage: 128 B of x per row, 64 B of weight
#define FW_BN 128                // output columns per block (4 waves x 32)
#define FW_ROW_B 128             // bytes per staged x row
#define FW_RING 4                // register ring slots (> prefetch depth, even)

typedef __bf16 fw_bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t fw_pack2(float a, float b) {
  return (uint32_t)(uint16_t)f32_to_bf16(a) | ((uint32_t)(uint16_t)f32_to_bf16(b) << 16);
}

// MT: 32-row activation tiles per block (1, 2 or 4). SPLIT: write the raw
// fp32 accumulators to this K slice's slab instead of the bf16 output.
// The body of both kernels below: one [M, N, K] problem, K slice ks.
template <int MT, bool SPLIT>
__device__ __forceinline__ void fw_body(
    bf16_t* __restrict__ out,            // [M, N]
    float* __restrict__ slabs,           // [splitk, M, N] (SPLIT only)
    const bf16_t* __restrict__ x,        // [M, K], row stride x_stride
    const unsigned char* __restrict__ q, // [N, K]
    const float* __restrict__ scale,     // [N]
    const bf16_t* __restrict__ bias,     // [N] or nullptr
    int M, int N, int K, long x_stride, int stages_per_slice, int ks) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int h = lane >> 5;
  const int r = lane & 31;

  const int n_blk = blockIdx.x * FW_BN + wv * 32;   // first column of this wave
  const int m_base = blockIdx.y * (MT * 32);

  const int n_stages = K / FW_BK;
  const int s_begin = ks * stages_per_slice;
  const int s_end = min(n_stages, s_begin + stages_per_slice);

  __shared__ __attribute__((aligned(16))) char smem[2 * MT * 32 * FW_ROW_B];
  const int BUF = MT * 32 * FW_ROW_B;

  // weight row of this lane, clamped into [0, N) (dropped at the store)
  const int n_row = min(n_blk + r, N - 1);
  const unsigned char* wsrc = q + (long)n_row * K + 16 * h;

  // x staging: thread t moves chunk (i * 256 + t): row = id >> 3, 16-B piece
  // id & 7 -- 8 consecutive lanes read one full 128-B line
  const bf16_t* xsrc[MT];
  int xdst[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int id = i * 256 + tid;
    const int row = id >> 3, ch = id & 7;
    const int m = min(m_base + row, M - 1);
    xsrc[i] = x + (long)m * x_stride + ch * 8;
    xdst[i] = row * FW_ROW_B + ((ch ^ (row & 7)) << 4);
  }

  f32x16 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = f32x16{};

  // Register ring, FW_RING slots: slot j % FW_RING holds stage j's weight
  // pieces and x chunks. FW_DEPTH stages are in flight beyond the one being
  // computed; loads return in order, so the only wait in the loop is the one
  // for the NEXT stage's x (written to LDS behind this stage's MFMAs), which
  // leaves FW_DEPTH - 1 stages outstanding. Every load is unconditional (a
  // stage index past the slice is clamped to its last stage): a branch
  // around a load would make the compiler drain the queue at the join.
  // (At MT = 4 a depth of 2 would fit three waves per SIMD instead of two;
  // measured, depth 3 at two waves is 5-10 % faster at M = 120 and 256.)
  constexpr int FW_DEPTH = 3;
  bf16x8_vec xr[FW_RING][MT];
  fw_u32x4 wr[FW_RING][2];

  auto load_stage = [&](int stage, int slot) {
    const unsigned char* p = wsrc + (long)stage * FW_BK;
    wr[slot][0] = *reinterpret_cast<const fw_u32x4*>(p);
    wr[slot][1] = *reinterpret_cast<const fw_u32x4*>(p + 32);
#pragma unroll
    for (int i = 0; i < MT; ++i)
      xr[slot][i] = *reinterpret_cast<const bf16x8_vec*>(xsrc[i] + (long)stage * FW_BK);
  };
  auto stx = [&](int buf, int slot) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
      *reinterpret_cast<bf16x8_vec*>(smem + buf * BUF + xdst[i]) = xr[slot][i];
  };

  if (s_begin < s_end) {
    const int last = s_end - 1;
#pragma unroll
    for (int i = 0; i < FW_DEPTH; ++i) load_stage(min(s_begin + i, last), i);
    stx(0, 0);
    __syncthreads();
    for (int base = s_begin; base < s_end; base += FW_RING) {
#pragma unroll
      for (int u = 0; u < FW_RING; ++u) {
        const int stage = base + u;
        if (stage >= s_end) break;
        load_stage(min(stage + FW_DEPTH, last), (u + FW_DEPTH) % FW_RING);
        const char* xb = smem + (u & 1) * BUF;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            fw_u32x4 a;
            uint32_t lo, hi;
            fw_cvt4(wr[u][p][2 * s], lo, hi);
            a[0] = lo; a[1] = hi;
            fw_cvt4(wr[u][p][2 * s + 1], lo, hi);
            a[2] = lo; a[3] = hi;
            const fw_bf16x8 af = __builtin_bit_cast(fw_bf16x8, a);
            const int ch = 4 * p + 2 * h + s;          // 16-B piece of the x row
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const int row = mt * 32 + r;
              const fw_bf16x8 xf = *reinterpret_cast<const fw_bf16x8*>(
                  xb + row * FW_ROW_B + ((ch ^ (row & 7)) << 4));
              acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, xf, acc[mt], 0, 0, 0);
            }
          }
        }
        stx((u + 1) & 1, (u + 1) % FW_RING);
        __syncthreads();
      }
    }
  }

  // epilogue: register g*4+i of the accumulator is column n = 8g + 4h + i
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m_base + mt * 32 + r;
    if (m >= M) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = n_blk + 8 * g + 4 * h;
      if (n >= N) continue;                         // N % 4 == 0: whole group
      if constexpr (SPLIT) {
        f32x4 v = {acc[mt][4 * g], acc[mt][4 * g + 1], acc[mt][4 * g + 2], acc[mt][4 * g + 3]};
        *reinterpret_cast<f32x4*>(slabs + ((long)ks * M + m) * N + n) = v;
      } else {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + n);
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = acc[mt][4 * g + i] * sc[i];
        if (bias != nullptr) {
          const bf16x4_vec b = *reinterpret_cast<const bf16x4_vec*>(bias + n);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] += bf16_to_f32(b[i]);
        }
        fw_u32x2 o = {fw_pack2(v[0], v[1]), fw_pack2(v[2], v[3])};
        *reinterpret_cast<fw_u32x2*>(out + (long)m * N + n) = o;
      }
    }
  }
}

template <int MT, bool SPLIT>
__global__ void __launch_bounds__(256) linear_fp8w_kernel(
    bf16_t* __restrict__ out, float* __restrict__ slabs, const bf16_t* __restrict__ x,
    const unsigned char* __restrict__ q, const float* __restrict__ scale,
    const bf16_t* __restrict__ bias, int M, int N, int K, long x_stride,
    int stages_per_slice) {
  fw_body<MT, SPLIT>(out, slabs, x, q, scale, bias, M, N, K, x_stride, stages_per_slice,
                     blockIdx.z);
}

// E independent [M, N, K] problems (the experts of a MoE layer) in one launch:
// blockIdx.z = e * splitk + ks. Expert e owns out[e] [M, N], q[e] [N, K],
// scale[e] [N], its splitk slabs and x + e * x_bstride (x_bstride == 0: one
// activation shared by all experts). Every clamp of the body is against M and
// N of expert e's own tensors, so a block never reads or writes a neighbour's.
template <int MT, bool SPLIT>
__global__ void __launch_bounds__(256) linear_fp8w_batched_kernel(
    bf16_t* __restrict__ out,            // [E, M, N]
    float* __restrict__ slabs,           // [E, splitk, M, N] (SPLIT only)
    const bf16_t* __restrict__ x,        // rows x_stride apart, experts x_bstride apart
    const unsigned char* __restrict__ q, // [E, N, K]
    const float* __restrict__ scale,     // [E, N]
    int M, int N, int K, long x_stride, long x_bstride, int stages_per_slice, int splitk) {
  const int e = blockIdx.z / splitk;
  const int ks = blockIdx.z - e * splitk;
  const long MN = (long)M * N;
  fw_body<MT, SPLIT>(out + e * MN, slabs + (long)e * splitk * MN, x + e * x_bstride,
                     q + (long)e * N * K, scale + (long)e * N, nullptr, M, N, K, x_stride,
                     stages_per_slice, ks);
}

// out[m, n] = bf16( (slab[0] + slab[1] + ... in slice order) * scale + bias );
// blockIdx.y is the expert of a batched call (0 otherwise).
extern "C" __global__ void __launch_bounds__(256) linear_fp8w_reduce_kernel(
    bf16_t* __restrict__ out, const float* __restrict__ slabs,
    const float* __restrict__ scale, const bf16_t* __restrict__ bias,
    long MN, int N, int splitk) {
  const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= MN) return;
  const int n = (int)(i4 % N);
  out += blockIdx.y * MN;
  slabs += (long)blockIdx.y * splitk * MN;
  scale += (long)blockIdx.y * N;
  f32x4 s = *reinterpret_cast<const f32x4*>(slabs + i4);
  for (int k = 1; k < splitk; ++k) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(slabs + (long)k * MN + i4);
    s += t;
  }
  const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + n);
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = s[i] * sc[i];
  if (bias != nullptr) {
    const bf16x4_vec b = *reinterpret_cast<const bf16x4_vec*>(bias + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += bf16_to_f32(b[i]);
  }
  fw_u32x2 o = {fw_pack2(v[0], v[1]), fw_pack2(v[2], v[3])};
  *reinterpret_cast<fw_u32x2*>(out + i4) = o;
}

// Large-M path: w[n, k] = bf16(fp32(q[n, k]) * scale[n]) into a reusable
// scratch; the GEMM then runs on the library (packed prefill stays on the
// tuned bf16 picks). One thread converts 16 weights.
extern "C" __global__ void __launch_bounds__(256) dequant_fp8w_kernel(
    bf16_t* __restrict__ w, const unsigned char* __restrict__ q,
    const float* __restrict__ scale, long n_vec, int K) {
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < n_vec; v += stride) {
    const long e = v * 16;
    const float sc = scale[e / K];                  // K % 16 == 0: one row
    const fw_u32x4 in = *reinterpret_cast<const fw_u32x4*>(q + e);
    fw_u32x4 o[2];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const fw_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)in[d], false);
      const fw_f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)in[d], true);
      o[d >> 1][2 * (d & 1)] = fw_pack2(a[0] * sc, a[1] * sc);
      o[d >> 1][2 * (d & 1) + 1] = fw_pack2(b[0] * sc, b[1] * sc);
    }
    *reinterpret_cast<fw_u32x4*>(w + e) = o[0];
    *reinterpret_cast<fw_u32x4*>(w + e + 8) = o[1];
  }
}

// Split-K slices for E [M, N, K] problems with 32*mt-row blocks. Fills the CUs
// when there are few column tiles, but keeps the fp32 slab traffic
// (splitk * M * N * 4 B per problem) under half the weight bytes (N * K).
static int fw_splitk(int mt, int E, int M, int N, int K, int n_cus) {
  const int m_blocks = (M + 32 * mt - 1) / (32 * mt);
  const int n_tiles = (N + FW_BN - 1) / FW_BN;
  const int n_stages = K / FW_BK;
  const int per_cu = mt == 4 ? 2 : 4;               // resident blocks wanted per CU
  int want = (int)(((long)n_cus * per_cu) / ((long)n_tiles * m_blocks * E));
  const int cap = K / (8 * M);                      // slab bytes <= weight bytes / 2
  want = std::min(std::min(want, cap), std::min(n_stages, 16));
  if (want <= 1) return 1;
  const int per = (n_stages + want - 1) / want;
  return (n_stages + per - 1) / per;                // no empty slice
}

// Row tile (mt) and split-K of a call: a pure function of the shape, the
// number of problems and the CU count, so the result bits never depend on
// anything else. M > 64 takes 128-row blocks unless that grid leaves CUs idle;
// then 64-row blocks give twice the blocks at half the MFMA and LDS work each
// (the second row block re-reads the weights through L2).
extern "C" void linear_fp8w_batched_plan(int E, int M, int N, int K, int n_cus, int* mt_out,
                                         int* splitk_out) {
  int mt = M <= 32 ? 1 : (M <= 64 ? 2 : 4);
  int splitk = fw_splitk(mt, E, M, N, K, n_cus);
  if (mt == 4) {
    const long blocks = (long)((N + FW_BN - 1) / FW_BN) * ((M + 127) / 128) * splitk * E;
    if (blocks < n_cus) {
      mt = 2;
      splitk = fw_splitk(mt, E, M, N, K, n_cus);
    }
  }
  *mt_out = mt;
  *splitk_out = splitk;
}

extern "C" void linear_fp8w_plan(int M, int N, int K, int n_cus, int* mt_out, int* splitk_out) {
  linear_fp8w_batched_plan(1, M, N, K, n_cus, mt_out, splitk_out);
}

extern "C" void launch_linear_fp8w(void* out, float* slabs, const void* x, const void* q,
                                   const float* scale, const void* bias, int M, int N, int K,
                                   long x_stride, int mt, int splitk, hipStream_t stream) {
  const int n_stages = K / FW_BK;
  const int per = (n_stages + splitk - 1) / splitk;
  const dim3 grid((N + FW_BN - 1) / FW_BN, (M + 32 * mt - 1) / (32 * mt), splitk);
#define FW_LAUNCH(MT_, SPLIT_)                                                          \
  hipLaunchKernelGGL((linear_fp8w_kernel<MT_, SPLIT_>), grid, dim3(256), 0, stream,     \
                     (bf16_t*)out, slabs, (const bf16_t*)x, (const unsigned char*)q,    \
                     scale, (const bf16_t*)bias, M, N, K, x_stride, per)
  if (splitk > 1) {
    if (mt == 1) FW_LAUNCH(1, true); else if (mt == 2) FW_LAUNCH(2, true); else FW_LAUNCH(4, true);
    const long MN = (long)M * N;
    const int blocks = (int)((MN / 4 + 255) / 256);
    hipLaunchKernelGGL(linear_fp8w_reduce_kernel, dim3(blocks), dim3(256), 0, stream,
                       (bf16_t*)out, (const float*)slabs, scale, (const bf16_t*)bias,
                       MN, N, splitk);
  } else {
    if (mt == 1) FW_LAUNCH(1, false); else if (mt == 2) FW_LAUNCH(2, false); else FW_LAUNCH(4, false);
  }
#undef FW_LAUNCH
}

extern "C" void launch_linear_fp8w_batched(void* out, float* slabs, const void* x,
                                           const void* q, const float* scale, int E, int M,
                                           int N, int K, long x_stride, long x_bstride, int mt,
                                           int splitk, hipStream_t stream) {
  const int n_stages = K / FW_BK;
  const int per = (n_stages + splitk - 1) / splitk;
  const dim3 grid((N + FW_BN - 1) / FW_BN, (M + 32 * mt - 1) / (32 * mt), E * splitk);
#define FW_LAUNCH(MT_, SPLIT_)                                                              \
  hipLaunchKernelGGL((linear_fp8w_batched_kernel<MT_, SPLIT_>), grid, dim3(256), 0, stream, \
                     (bf16_t*)out, slabs, (const bf16_t*)x, (const unsigned char*)q, scale, \
                     M, N, K, x_stride, x_bstride, per, splitk)
  if (splitk > 1) {
    if (mt == 1) FW_LAUNCH(1, true); else if (mt == 2) FW_LAUNCH(2, true); else FW_LAUNCH(4, true);
    const long MN = (long)M * N;
    const int blocks = (int)((MN / 4 + 255) / 256);
    hipLaunchKernelGGL(linear_fp8w_reduce_kernel, dim3(blocks, E), dim3(256), 0, stream,
                       (bf16_t*)out, (const float*)slabs, scale, (const bf16_t*)nullptr,
                       MN, N, splitk);
  } else {
    if (mt == 1) FW_LAUNCH(1, false); else if (mt == 2) FW_LAUNCH(2, false); else FW_LAUNCH(4, false);
  }
#undef FW_LAUNCH
}

extern "C" void launch_dequant_fp8w(void* w, const void* q, const float* scale, long numel,
                                    int K, hipStream_t stream) {
  const long n_vec = numel / 16;
  const int blocks = (int)std::min<long>((n_vec + 255) / 256, 8192);
  hipLaunchKernelGGL(dequant_fp8w_kernel, dim3(blocks), dim3(256), 0, stream,
                     (bf16_t*)w, (const unsigned char*)q, scale, n_vec, K);
}
