// Batched paged-KV block copies for gfx950: every (src_block, dst_block) pair
// of a fork batch, for all layers and for both arrays of a cache (K and V, or
// the two fp8 scale arrays), in ONE launch.
//
// The arrays are [L, NB, ...] with `block_bytes` per block and `layer_stride`
// bytes between layers. In production one layer spans more than 2^31 bytes,
// so every offset is formed in 64 bits. A work unit is one block of one layer
// of one array; workgroups stride over the units (capped grid) and the 256
// threads of a workgroup stride over the block in lanes of VEC bytes.
//
// One source may feed many destinations; the host guarantees that no block is
// both a source and a destination of the same call, so units never race.

#include "launch.h"

#define KV_COPY_MAX_GRID 2048

template <typename VEC>
__global__ void __launch_bounds__(256) copy_kv_blocks_kernel(
    unsigned char* __restrict__ a_base, unsigned char* __restrict__ b_base,
    const int* __restrict__ src, const int* __restrict__ dst, int n_pairs, int n_layers,
    int64_t layer_stride, int64_t block_bytes) {
  const int64_t units = (int64_t)n_pairs * n_layers * 2;
  const int64_t nvec = block_bytes / (int64_t)sizeof(VEC);
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int which = (int)(u & 1);
    const int64_t pl = u >> 1;
    const int layer = (int)(pl % n_layers);
    const int pair = (int)(pl / n_layers);
    unsigned char* base = (which ? b_base : a_base) + (int64_t)layer * layer_stride;
    const VEC* s = reinterpret_cast<const VEC*>(base + (int64_t)src[pair] * block_bytes);
    VEC* d = reinterpret_cast<VEC*>(base + (int64_t)dst[pair] * block_bytes);
    // four loads in flight per thread before the first store
    const int64_t bd = blockDim.x;
    int64_t i = threadIdx.x;
    for (; i + 3 * bd < nvec; i += 4 * bd) {
      const VEC v0 = s[i], v1 = s[i + bd], v2 = s[i + 2 * bd], v3 = s[i + 3 * bd];
      d[i] = v0;
      d[i + bd] = v1;
      d[i + 2 * bd] = v2;
      d[i + 3 * bd] = v3;
    }
    for (; i < nvec; i += bd) d[i] = s[i];
  }
}

// vec_bytes: 16, 4 or 1 -- the widest lane that divides block_bytes,
// layer_stride and both base addresses (chosen by the binding).
extern "C" void launch_copy_kv_blocks(void* a_base, void* b_base, const int* src, const int* dst,
                                      int n_pairs, int n_layers, int64_t layer_stride,
                                      int64_t block_bytes, int vec_bytes, hipStream_t stream) {
  const int64_t units = (int64_t)n_pairs * n_layers * 2;
  if (units <= 0 || block_bytes <= 0) return;
  const int grid = (int)(units < KV_COPY_MAX_GRID ? units : KV_COPY_MAX_GRID);
  unsigned char* a = reinterpret_cast<unsigned char*>(a_base);
  unsigned char* b = reinterpret_cast<unsigned char*>(b_base);
  if (vec_bytes == 16) {
    hipLaunchKernelGGL(copy_kv_blocks_kernel<fw_u32x4>, dim3(grid), dim3(256), 0, stream,
                       a, b, src, dst, n_pairs, n_layers, layer_stride, block_bytes);
  } else if (vec_bytes == 4) {
    hipLaunchKernelGGL(copy_kv_blocks_kernel<unsigned int>, dim3(grid), dim3(256), 0, stream,
                       a, b, src, dst, n_pairs, n_layers, layer_stride, block_bytes);
  } else {
    hipLaunchKernelGGL(copy_kv_blocks_kernel<unsigned char>, dim3(grid), dim3(256), 0, stream,
                       a, b, src, dst, n_pairs, n_layers, layer_stride, block_bytes);
  }
}
