// MXFP4 weights -> the bf16 fragment image the MFMA GEMMs read (the one-copy MXFP4 model: the codes
// are the only resident copy and a projection is dequantised into a reusable scratch right before
// a GEMM without an MXFP4 arm reads it).  A pure stream: 16 B of codes and 4 B of scales in, 64 B out.
#include "common.h"

namespace dab {

// One lane per 16 B of codes.  MXFP4 fragment f = (sb nk + j) G + g (ops.shuffle_weights_mxfp4, nk =
// K / 128, G = group), lane l: bytes 4c .. 4c + 3 are the lane's operand of the 32-deep chunk 4j + c, so
// they become lane l's 16 B of the bf16 fragment ((sb 4 nk + 4j + c) G + g) (ops.shuffle_weights).  The
// scale dword of row l & 15 (ops.shuffle_scales_mxfp4: [N/16][nk][16][4], block sb G + g) holds the
// four chunks' bytes; the four lane quadrants of a row read the same dword.
template <bool NT>
__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(const uint8_t* __restrict__ codes,
                                                            const uint8_t* __restrict__ scales,
                                                            bf16* __restrict__ out, size_t nlane, uint32_t nk,
                                                            uint32_t G) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nlane; i += (size_t)gridDim.x * 256) {
    const uint32_t lane = (uint32_t)(i & 63);
    const size_t f = i >> 6, t = f / G, g = f - t * G, sb = t / nk, j = t - sb * nk;
    const u32x4 d = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(codes) + i);  // read once
    const uint32_t sc = *reinterpret_cast<const uint32_t*>(scales + (((sb * G + g) * nk + j) * 16 + (lane & 15)) * 4);
    bf16* dst = out + ((sb * 4 * nk + 4 * j) * G + g) * 512 + lane * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const u32x4 o = __builtin_bit_cast(u32x4, fp4x8_bf16(d[c], exp_scale((sc >> (8 * c)) & 0xff)));
      u32x4* q = reinterpret_cast<u32x4*>(dst + (size_t)c * G * 512);
      if constexpr (NT) __builtin_nontemporal_store(o, q);
      else *q = o;
    }
  }
}

// store policy of the image: 0 = default (the consumer GEMM reads it next), 1 = non-temporal; A/B switch
static int g_dequant_nt = 0;
void weight_dequant_mxfp4_set_nt(int on) { g_dequant_nt = on != 0; }
int weight_dequant_mxfp4_nt() { return g_dequant_nt; }

int weight_dequant_mxfp4(const void* codes, const void* scales, void* out, long N, long K, int group, int grid_cap,
                         hipStream_t s) {
  if (N <= 0 || K <= 0 || group < 1 || grid_cap < 0 || K % 128 || N % (16L * group)) return hipErrorInvalidValue;
  if (!codes || !scales || !out || (uintptr_t)codes % 16 || (uintptr_t)scales % 4 || (uintptr_t)out % 16)
    return hipErrorInvalidValue;
  if (group > 1 && (size_t)N * (size_t)K * 2 >= (size_t(1) << 31)) return hipErrorInvalidValue;
  const size_t nlane = (size_t)N * (size_t)K / 32;
  size_t blocks = (nlane + 255) / 256;
  // 8 workgroups of 4 waves fill a CU's wave slots; more only adds launch ramp to a memory-bound loop
  static const int per_chip = [] {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return 8 * cus;
  }();
  const size_t cap = grid_cap > 0 ? (size_t)grid_cap : (size_t)per_chip;
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks), wg(256);
  if (g_dequant_nt)
    hipLaunchKernelGGL(mxfp4_dequant_kernel<true>, grid, wg, 0, s, (const uint8_t*)codes, (const uint8_t*)scales,
                       (bf16*)out, nlane, (uint32_t)(K / 128), (uint32_t)group);
  else
    hipLaunchKernelGGL(mxfp4_dequant_kernel<false>, grid, wg, 0, s, (const uint8_t*)codes, (const uint8_t*)scales,
                       (bf16*)out, nlane, (uint32_t)(K / 128), (uint32_t)group);
  return hipGetLastError();
}

}  // namespace dab
