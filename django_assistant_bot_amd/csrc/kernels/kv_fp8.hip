// FP8 paged KV cache (opt-in, D = 128): per (token, kv head) row 128 OCP e4m3fn bytes and one E8M0
// exponent byte b (value = byte x 2^(b - 127)), K and V alike.
//
//   rope_kv_fp8_kernel      : RoPE + quantising cache write (the FP8 form of rope_kv_kernel)
//   kv_fp8_dequant_kernel   : bf16 image of a list of blocks (the prefill attention reads a scratch;
//                             fp8x16_dequant of common.h, as the index's dequantiser)
//   paged_decode_fp8_kernel : paged_decode_kernel's structure on 128-byte rows, FP8 -> bf16 in
//                             registers (exact), bf16 MFMA with fp32 accumulation
//
// Data layout [num_blocks, Hkv, block_size, 128] uint8, exponents [num_blocks, Hkv, block_size] uint8.
// A power-of-two scale makes every dequantised value bf16-exact, so the exponents can be applied to
// the fp32 scores (K) and to P before its bf16 rounding (V) instead of to the converted operands:
// the same numbers as bf16 MFMAs on the dequantised cache, barring fp32 under / overflow.
#include "common.h"
#include "launchers.h"

namespace dab {

namespace {

constexpr float kNegInfF = -__builtin_huge_valf();

// (fp8x8_bf16 / exp_scale: common.h, shared with the FP8-weight decode GEMM)

// Exponent byte of a row whose largest |bf16 bits| is `a` (sign cleared): amax = 1.M x 2^(E - 127),
// the smallest power of two 2^e with amax / 2^e <= 448 is e = E - 135, or E - 134 when 1.M > 1.75.
__device__ __forceinline__ uint32_t row_exponent(uint32_t a) {
  if (a == 0) return 127;
  const int b = (int)(a >> 7) - 8 + ((a & 0x7f) > 0x60 ? 1 : 0);
  return (uint32_t)min(max(b, 1), 254);
}

// 8 bf16-exact values times `inv` (exact), clamped to +-448 -> 8 e4m3fn bytes, nearest-even
__device__ __forceinline__ u32x2 quant8(const float (&x)[8], float inv, bool zero) {
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = fminf(fmaxf(x[j] * inv, -448.f), 448.f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  return zero ? u32x2{0u, 0u} : u32x2{(uint32_t)lo, (uint32_t)hi};
}

}  // namespace

// The thread -> (token, head, 8-pair chunk) map, inputs and q output of rope_kv_kernel (q bit for
// bit: the same rope_chunk and pack8).  The 8 consecutive threads of a k / v head row hold its 128
// values; the row's amax is a reduction over those 8 lanes, so no lane leaves before the shuffles
// (threads past the end recompute the last row and store nothing).
template <typename ST>
__global__ __launch_bounds__(256) void rope_kv_fp8_kernel(const bf16* __restrict__ qkv, int ld,
                                                          const int* __restrict__ positions,
                                                          const float2* __restrict__ cos_sin, bf16* __restrict__ q_out,
                                                          uint8_t* __restrict__ k_data, uint8_t* __restrict__ k_exp,
                                                          uint8_t* __restrict__ v_data, uint8_t* __restrict__ v_exp,
                                                          const int64_t* __restrict__ slots, int T, int Hq, int Hkv,
                                                          int block_size, const ST* __restrict__ slabs, int S,
                                                          long slab_stride) {
  constexpr int D = 128, half = 64, per_head = 8;
  const int heads = Hq + 2 * Hkv;
  const int h0 = q_out ? 0 : Hq;
  const int hrun = heads - h0;
  const size_t total = (size_t)T * hrun * per_head;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = gid < total;
  const size_t idx = live ? gid : total - 1;
  const int c = (int)(idx % per_head);
  const size_t th = idx / per_head;
  const int h = h0 + (int)(th % hrun);
  const int t = (int)(th / hrun);
  const int i0 = c * 8;
  float2 cs[8];
  rope_cs(cos_sin, positions[t], half, i0, cs);
  const int64_t slot = h >= Hq ? slots[t] : 0;
  float x1[8], x2[8];
  rope_chunk(qkv, slabs, S, slab_stride, ld, t, h, D, i0, cs, h < Hq + Hkv, x1, x2);
  const u32x4 p1 = pack8(x1), p2 = pack8(x2);  // what the bf16 cache would hold
  uint32_t a = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a = max(a, max(p1[j] & 0x7fffu, (p1[j] >> 16) & 0x7fffu));
    a = max(a, max(p2[j] & 0x7fffu, (p2[j] >> 16) & 0x7fffu));
  }
  a = max(a, (uint32_t)__shfl_xor((int)a, 1, 64));
  a = max(a, (uint32_t)__shfl_xor((int)a, 2, 64));
  a = max(a, (uint32_t)__shfl_xor((int)a, 4, 64));
  if (!live) return;
  if (h < Hq) {
    bf16* dst = q_out + ((size_t)t * Hq + h) * D;
    *reinterpret_cast<u32x4*>(dst + i0) = p1;
    *reinterpret_cast<u32x4*>(dst + i0 + half) = p2;
    return;
  }
  if (slot < 0) return;
  const int64_t blk = slot / block_size, off = slot - blk * block_size;
  const bool is_k = h < Hq + Hkv;
  const int kh = is_k ? h - Hq : h - Hq - Hkv;
  const size_t row = ((size_t)blk * Hkv + kh) * block_size + off;
  const uint32_t b = row_exponent(a);
  const float inv = __uint_as_float((254u - b) << 23);  // 2^-(b - 127)
  float r1[8], r2[8];
  unpack8(p1, r1);
  unpack8(p2, r2);
  uint8_t* dst = (is_k ? k_data : v_data) + row * D;
  *reinterpret_cast<u32x2*>(dst + i0) = quant8(r1, inv, a == 0);
  *reinterpret_cast<u32x2*>(dst + i0 + half) = quant8(r2, inv, a == 0);
  if (c == 0) (is_k ? k_exp : v_exp)[row] = (uint8_t)b;
}

// One lane per 16 bytes of a row: out[i] ([Hkv, block_size, 128] bf16) = block ids[i], K and V.
__global__ __launch_bounds__(256) void kv_fp8_dequant_kernel(const uint8_t* __restrict__ k_data,
                                                             const uint8_t* __restrict__ k_exp,
                                                             const uint8_t* __restrict__ v_data,
                                                             const uint8_t* __restrict__ v_exp,
                                                             const int* __restrict__ ids, bf16* __restrict__ k_out,
                                                             bf16* __restrict__ v_out, size_t nchunks,
                                                             int rows_per_block) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (size_t)gridDim.x * 256) {
    const size_t orow = i >> 3;
    const int c = (int)(i & 7);
    const size_t ob = orow / rows_per_block;
    const size_t srow = (size_t)ids[ob] * rows_per_block + (orow - ob * rows_per_block);
    const u32x4 kd = *reinterpret_cast<const u32x4*>(k_data + srow * 128 + 16 * c);
    const u32x4 vd = *reinterpret_cast<const u32x4*>(v_data + srow * 128 + 16 * c);
    u32x4 ko[2], vo[2];
    fp8x16_dequant(kd, exp_scale(k_exp[srow]), ko);
    fp8x16_dequant(vd, exp_scale(v_exp[srow]), vo);
    u32x4* kp = reinterpret_cast<u32x4*>(k_out + orow * 128 + 16 * c);
    u32x4* vp = reinterpret_cast<u32x4*>(v_out + orow * 128 + 16 * c);
    kp[0] = ko[0];
    kp[1] = ko[1];
    vp[0] = vo[0];
    vp[1] = vo[1];
  }
}

// -----------------------------------------------------------------------------------------------
// Paged decode over the FP8 cache: paged_decode_kernel<128, true, true, NSLOT> (attention.hip) with
// 32-key x 128-B sub-tiles.  What differs:
//   * LDS image: byte offset of 16-B chunk c of row r is r 128 + 16 (c ^ f(r)), f(r) = (r & 6) ^
//     ((r >> 3) & 1): the 16 rows of a K row read (ds_read_b128) land on 16 different bank groups,
//     and the 8 rows x 32 B of a transposed V read of one 32-lane half cover all 64 banks once.
//     A 1 KB LDS-DMA piece is 8 rows; lane l of piece i fetches logical chunk (l & 7) ^ f(8 i + l / 8).
//   * S^T = K Q^T: a lane's 16 K bytes are dims 64 h + 16 g .. + 15 (two k-steps of one ds_read_b128;
//     the q fragments are loaded in the same dim order -- the contraction runs over all 128 anyway).
//   * O^T = V^T P^T: ds_read_b64_tr_b16 on BYTE PAIRS: lane li of a 16-lane group receives dims
//     (32 u + 2 li, + 1) of 4 keys; a v_perm splits the pair, so MFMA tile t = 2 u + par holds
//     dim 32 u + 2 row + par in its row `row` (undone where o[] is written to LDS).
//   * the K exponents scale the scores, the V exponents scale P before its bf16 rounding (the row
//     sum keeps the unscaled p); a sub-tile's 32 + 32 exponent bytes are 4 dword loads per lane,
//     issued with the sub-tile's copy.

struct DecodeFp8Params {
  const bf16* q;
  const uint8_t* k_data;
  const uint8_t* v_data;
  const uint8_t* k_exp;
  const uint8_t* v_exp;
  const int* block_tables;
  int max_blocks, block_size;
  const int* ctx_lens;
  bf16* out;
  float* part_o;
  float* part_m;
  float* part_l;
  int* counters;
  const int* order;
  int Hq, Hkv, part_size, max_parts;
  float scale_log2;
};

__device__ __forceinline__ int fswz(int r, int c) { return r * 128 + 16 * (c ^ ((r & 6) ^ ((r >> 3) & 1))); }

template <int NSLOT>
__global__ __launch_bounds__(256, NSLOT == 1 ? 2 : 1) void paged_decode_fp8_kernel(DecodeFp8Params p, int total_items) {
  constexpr int D = 128;
  constexpr int KT = 32;
  constexpr int NKK = D / 32;
  constexpr int NTD = D / 16;
  constexpr int SUB_BYTES = KT * D;
  constexpr int RED_BYTES = 4 * 16 * D * 4 + 2 * 4 * 16 * 4;
  constexpr int STAGE_BYTES = 4 * 2 * SUB_BYTES * NSLOT;
  constexpr int AREA_BYTES = STAGE_BYTES > RED_BYTES + 16 ? STAGE_BYTES : RED_BYTES + 16;
  __shared__ __attribute__((aligned(16))) char smem[AREA_BYTES];
  int* last_flag = reinterpret_cast<int*>(smem + RED_BYTES);

  const int G = p.Hq / p.Hkv;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* const slot0 = smem + w * 2 * SUB_BYTES * NSLOT;
  char* ks = slot0;
  char* vs = ks + SUB_BYTES;

  const int attn_blocks = gridDim.x;
  const int BH = total_items / p.max_parts;
  int maxc = 0;
  for (int i = lane; i < BH / p.Hkv; i += 64) maxc = max(maxc, p.ctx_lens[i]);
#pragma unroll
  for (int off = 32; off; off >>= 1) maxc = max(maxc, __shfl_xor(maxc, off));
  maxc = __builtin_amdgcn_readfirstlane(maxc);
  const int live_items = min(p.max_parts, (maxc + p.part_size - 1) / p.part_size) * BH;
  for (int item = blockIdx.x; item < live_items; item += attn_blocks) {
    const int part = item / BH;
    const int bh = item - part * BH;
    const int hk = bh % p.Hkv, b = p.order ? p.order[bh / p.Hkv] : bh / p.Hkv;
    const int ctx = p.ctx_lens[b];
    const int k_begin = part * p.part_size;
    if (k_begin >= ctx) continue;
    const int k_end = min(ctx, k_begin + p.part_size);

    // q fragment of k-step kk: dims 64 (kk / 2) + 16 g + 8 (kk % 2) .. + 7 (the order of the K bytes)
    bf16x8 qf[NKK];
    {
      const bool qv = li < G;
      const bf16* qrow = p.q + ((size_t)b * p.Hq + hk * G + (qv ? li : 0)) * D;
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        qf[kk] = qv ? *reinterpret_cast<const bf16x8*>(qrow + 64 * (kk >> 1) + 16 * g + 8 * (kk & 1)) : z;
      }
    }

    f32x4 o[NTD];
#pragma unroll
    for (int t = 0; t < NTD; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;
    const int k_last = ((k_end - 1) / KT) * KT;

    // ke / ve: exponent bytes of keys 16 m + 4 g + r (byte r of word m) of the sub-tile
    auto compute = [&](const int k0, const uint32_t (&ke)[2], const uint32_t (&ve)[2]) {
      __builtin_amdgcn_wave_barrier();
      f32x4 s[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        s[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const u32x4 kb = *reinterpret_cast<const u32x4*>(ks + fswz(16 * m + li, 4 * h + g));
          s[m] = mfma16(fp8x8_bf16(kb[0], kb[1]), qf[2 * h], s[m]);
          s[m] = mfma16(fp8x8_bf16(kb[2], kb[3]), qf[2 * h + 1], s[m]);
        }
      }
      float mx = kNegInfF;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + 16 * m + 4 * g + r;
          float v = s[m][r] * exp_scale((ke[m] >> (8 * r)) & 0xffu) * p.scale_log2;
          if (key >= k_end) v = kNegInfF;
          s[m][r] = v;
          mx = fmaxf(mx, v);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = exp2f(m_run - m_new);
      float ls = 0.f;
      bf16x8 pb;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + 16 * m + 4 * g + r;
          const float e = exp2f(s[m][r] - m_new);
          ls += e;
          // masked keys: exactly 0 whatever exponent byte the unused slot holds
          const float pv = key >= k_end ? 0.f : e * exp_scale((ve[m] >> (8 * r)) & 0xffu);
          pb[4 * m + r] = (short)f2bf(pv);
        }
      }
      l_run = l_run * alpha + ls;
      m_run = m_new;
      const int qq = li >> 2, pp = li & 3;
#pragma unroll
      for (int u = 0; u < NTD / 2; ++u) {
        o[2 * u] *= alpha;
        o[2 * u + 1] *= alpha;
        const int ch = 2 * u + (pp >> 1);
        const int boff = 8 * (pp & 1);
        const u32x2 lo = __builtin_bit_cast(u32x2, ds_read_tr16(vs + fswz(4 * g + qq, ch) + boff));
        const u32x2 hi = __builtin_bit_cast(u32x2, ds_read_tr16(vs + fswz(16 + 4 * g + qq, ch) + boff));
        // lo / hi: 4 keys x (dim 32 u + 2 li, + 1) -> the even dims' 8 keys, the odd dims' 8 keys
        const uint32_t e_lo = __builtin_amdgcn_perm(lo[1], lo[0], 0x06040200u);
        const uint32_t e_hi = __builtin_amdgcn_perm(hi[1], hi[0], 0x06040200u);
        const uint32_t o_lo = __builtin_amdgcn_perm(lo[1], lo[0], 0x07050301u);
        const uint32_t o_hi = __builtin_amdgcn_perm(hi[1], hi[0], 0x07050301u);
        o[2 * u] = mfma16(fp8x8_bf16(e_lo, e_hi), pb, o[2 * u]);
        o[2 * u + 1] = mfma16(fp8x8_bf16(o_lo, o_hi), pb, o[2 * u + 1]);
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the slot's LDS reads returned
      __builtin_amdgcn_wave_barrier();
    };

    const int kw = k_begin + w * KT;
    const int drow = lane >> 3;
    auto blk_at = [&](int k0) { return p.block_tables[(size_t)b * p.max_blocks + min(k0, k_last) / p.block_size]; };
    // 8 LDS-DMA pieces (K and V, 8 rows each) + 4 exponent dwords: 12 vector-memory operations
    auto fetch = [&](int k0, int blk, uint32_t (&ke)[2], uint32_t (&ve)[2]) {
      const int kc = min(k0, k_last);
      const size_t row0 = ((size_t)blk * p.Hkv + hk) * p.block_size + (kc % p.block_size);
      const int bytes = k0 > k_last ? 0 : min(KT, k_end - k0) * D;
      // (a sub-tile starts on a multiple of 32 inside its block: its 32 exponent bytes exist; first,
      // so that they return ahead of the copy they were issued with)
      const uint32_t* kep = reinterpret_cast<const uint32_t*>(p.k_exp + row0) + g;
      const uint32_t* vep = reinterpret_cast<const uint32_t*>(p.v_exp + row0) + g;
      ke[0] = __builtin_nontemporal_load(kep);
      ke[1] = __builtin_nontemporal_load(kep + 4);
      ve[0] = __builtin_nontemporal_load(vep);
      ve[1] = __builtin_nontemporal_load(vep + 4);
      const auto kd = __builtin_amdgcn_make_buffer_rsrc((void*)(p.k_data + row0 * D), 0, bytes, 0x00020000);
      const auto vd = __builtin_amdgcn_make_buffer_rsrc((void*)(p.v_data + row0 * D), 0, bytes, 0x00020000);
#pragma unroll
      for (int i = 0; i < KT / 8; ++i) {
        const int row = 8 * i + drow;
        const unsigned off = (unsigned)(row * 128 + 16 * ((lane & 7) ^ ((row & 6) ^ ((row >> 3) & 1))));
        __builtin_amdgcn_raw_ptr_buffer_load_lds(kd, (__attribute__((address_space(3))) void*)(ks + i * 1024), 16, off, 0,
                                                 0, 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(vd, (__attribute__((address_space(3))) void*)(vs + i * 1024), 16, off, 0,
                                                 0, 2);
      }
    };
    uint32_t ke[2], ve[2];
    if constexpr (NSLOT == 2) {
      const int n_sub = kw < k_end ? (k_end - kw + 4 * KT - 1) / (4 * KT) : 0;  // <= 64 (launcher)
      int myblk = lane < n_sub ? blk_at(kw + lane * 4 * KT) : 0;  // lane i: sub-tile i's block
      // q (issued before it) and the block ids have arrived before the sub-tile loop: otherwise the
      // wait for them lands inside the loop as a vmcnt(0), which also waits for the next sub-tile's copy
      asm volatile("" : "+v"(myblk));
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) asm volatile("" : "+v"(qf[kk]));
      uint32_t kn[2], vn[2];
      auto use_slot = [&](int i) {
        ks = slot0 + (i & 1) * 2 * SUB_BYTES;
        vs = ks + SUB_BYTES;
      };
      if (n_sub > 0) {
        use_slot(0);
        fetch(kw, __builtin_amdgcn_readlane(myblk, 0), ke, ve);
      }
      for (int i = 0; i < n_sub; ++i) {
        if (i + 1 < n_sub) {
          use_slot(i + 1);  // the slot sub-tile i - 1 was read from (its MFMAs consumed it)
          fetch(kw + (i + 1) * 4 * KT, __builtin_amdgcn_readlane(myblk, i + 1), kn, vn);
          asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // sub-tile i's 12 operations landed
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        use_slot(i);
        compute(kw + i * 4 * KT, ke, ve);
        if (i + 1 < n_sub) {
          ke[0] = kn[0], ke[1] = kn[1];
          ve[0] = vn[0], ve[1] = vn[1];
        }
      }
    } else {
      int blk = __builtin_amdgcn_readfirstlane(blk_at(kw));
      for (int k0 = kw; k0 < k_end; k0 += 4 * KT) {
        fetch(k0, blk, ke, ve);
        blk = blk_at(k0 + 4 * KT);  // issued right behind the copy: returns with it
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this sub-tile's 12 operations landed
        compute(k0, ke, ve);
        blk = __builtin_amdgcn_readfirstlane(blk);
      }
    }

    // combine the 4 waves of the workgroup through LDS
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    __syncthreads();
    float* ored = reinterpret_cast<float*>(smem);  // [4][16][D]
    float* mred = ored + 4 * 16 * D;               // [4][16]
    float* lred = mred + 4 * 16;                   // [4][16]
    // o[2 u + par][r] is dim 32 u + 2 (4 g + r) + par: 8 consecutive dims from 32 u + 8 g
#pragma unroll
    for (int u = 0; u < NTD / 2; ++u) {
      float* dst = ored + (w * 16 + li) * D + 32 * u + 8 * g;
      *reinterpret_cast<f32x4*>(dst) = f32x4{o[2 * u][0], o[2 * u + 1][0], o[2 * u][1], o[2 * u + 1][1]};
      *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[2 * u][2], o[2 * u + 1][2], o[2 * u][3], o[2 * u + 1][3]};
    }
    if (g == 0) {
      mred[w * 16 + li] = m_run;
      lred[w * 16 + li] = l_run;
    }
    __syncthreads();
    const int np = min(p.max_parts, div_up(ctx, p.part_size));
    const bool direct = np == 1;
    for (int e = tid; e < G * D; e += 256) {
      const int qh = e / D, d = e % D;
      float M = -1e30f;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) M = fmaxf(M, mred[ww * 16 + qh]);
      float L = 0.f, O = 0.f;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const float f = exp2f(mred[ww * 16 + qh] - M);
        L += f * lred[ww * 16 + qh];
        O += f * ored[(ww * 16 + qh) * D + d];
      }
      const size_t hq = (size_t)b * p.Hq + hk * G + qh;
      if (direct) {
        p.out[hq * D + d] = f2bf(L > 0.f ? O / L : 0.f);
      } else {
        const size_t pi = hq * p.max_parts + part;
        __hip_atomic_store(p.part_o + pi * D + d, O, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (d == 0) {
          __hip_atomic_store(p.part_m + pi, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(p.part_l + pi, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    if (!direct) {
      // the in-launch last-arriver combine of paged_decode_kernel, same workspace and counters
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        const int ci = b * p.Hkv + hk;
        const int prev = __hip_atomic_fetch_add(p.counters + ci, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = prev == np - 1;
        if (last) __hip_atomic_store(p.counters + ci, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last_flag = last;
      }
      __syncthreads();
      if (*last_flag) {
        auto ld = [](const float* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        for (int e = tid; e < G * D; e += 256) {
          const int qh = e / D, d = e % D;
          const size_t hq = (size_t)b * p.Hq + hk * G + qh;
          const size_t base = hq * p.max_parts;
          float M = -1e30f;
          for (int i = 0; i < np; ++i) M = fmaxf(M, ld(p.part_m + base + i));
          float L = 0.f, O = 0.f;
          for (int i = 0; i < np; ++i) {
            const float f = exp2f(ld(p.part_m + base + i) - M);
            L += f * ld(p.part_l + base + i);
            O += f * ld(p.part_o + (base + i) * D + d);
          }
          p.out[hq * D + d] = f2bf(L > 0.f ? O / L : 0.f);
        }
      }
    }
    __syncthreads();  // LDS is restaged by the next item
  }
}

// -----------------------------------------------------------------------------------------------

int rope_kv_write_fp8(const void* qkv, int ld, const int* positions, const void* cos_sin, void* q_out, void* k_data,
                      void* k_exp, void* v_data, void* v_exp, const int64_t* slots, int T, int Hq, int Hkv, int D,
                      int block_size, hipStream_t s, const void* slabs, int S, long slab_stride, int slab_bf16) {
  if (T <= 0) return 0;
  if (D != 128 || ld % 8 || (slabs && (S < 1 || slab_stride % 8)) || (!slabs && !qkv)) return hipErrorInvalidValue;
  const size_t total = (size_t)T * (q_out ? Hq + 2 * Hkv : 2 * Hkv) * 8;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (slabs && slab_bf16)
    hipLaunchKernelGGL(rope_kv_fp8_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)qkv, ld, positions,
                       (const float2*)cos_sin, (bf16*)q_out, (uint8_t*)k_data, (uint8_t*)k_exp, (uint8_t*)v_data,
                       (uint8_t*)v_exp, slots, T, Hq, Hkv, block_size, (const bf16*)slabs, S, slab_stride);
  else
    hipLaunchKernelGGL(rope_kv_fp8_kernel<float>, grid, dim3(256), 0, s, (const bf16*)qkv, ld, positions,
                       (const float2*)cos_sin, (bf16*)q_out, (uint8_t*)k_data, (uint8_t*)k_exp, (uint8_t*)v_data,
                       (uint8_t*)v_exp, slots, T, Hq, Hkv, block_size, (const float*)slabs, S, slab_stride);
  return hipGetLastError();
}

int kv_fp8_dequant_blocks(const void* k_data, const void* k_exp, const void* v_data, const void* v_exp,
                          const int* block_ids, int n, void* k_out, void* v_out, int Hkv, int block_size, int D,
                          hipStream_t s) {
  if (n <= 0) return 0;
  if (D != 128 || Hkv < 1 || block_size < 1) return hipErrorInvalidValue;
  const int rows_per_block = Hkv * block_size;
  const size_t nchunks = (size_t)n * rows_per_block * 8;
  size_t g = (nchunks + 255) / 256;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(kv_fp8_dequant_kernel, dim3((unsigned)g), dim3(256), 0, s, (const uint8_t*)k_data,
                     (const uint8_t*)k_exp, (const uint8_t*)v_data, (const uint8_t*)v_exp, block_ids, (bf16*)k_out,
                     (bf16*)v_out, nchunks, rows_per_block);
  return hipGetLastError();
}

int paged_decode_attention_fp8(const void* q, const void* k_data, const void* k_exp, const void* v_data,
                               const void* v_exp, const int* block_tables, int max_blocks, int block_size,
                               const int* ctx_lens, void* out, float* part_o, float* part_m, float* part_l,
                               int* counters, int batch, int Hq, int Hkv, int D, int part_size, int max_parts,
                               float scale, hipStream_t s, const int* order) {
  if (batch <= 0) return 0;
  if (D != 128) return hipErrorInvalidValue;
  if (Hq % Hkv || Hq / Hkv > 16 || part_size % 128 || max_parts < 1 || block_size % 32) return hipErrorInvalidValue;
  if (max_parts > 1 && !counters) return hipErrorInvalidValue;
  if (!q) return hipErrorInvalidValue;
  DecodeFp8Params prm;
  prm.q = (const bf16*)q;
  prm.k_data = (const uint8_t*)k_data;
  prm.v_data = (const uint8_t*)v_data;
  prm.k_exp = (const uint8_t*)k_exp;
  prm.v_exp = (const uint8_t*)v_exp;
  prm.block_tables = block_tables;
  prm.max_blocks = max_blocks;
  prm.block_size = block_size;
  prm.ctx_lens = ctx_lens;
  prm.out = (bf16*)out;
  prm.part_o = part_o;
  prm.part_m = part_m;
  prm.part_l = part_l;
  prm.counters = counters;
  prm.order = order;
  prm.Hq = Hq;
  prm.Hkv = Hkv;
  prm.part_size = part_size;
  prm.max_parts = max_parts;
  prm.scale_log2 = scale * 1.4426950408889634f;
  const int total_items = max_parts * Hkv * batch;
  dim3 grid(total_items < 2048 ? total_items : 2048);
  // the dispatch of paged_decode_attention: two LDS slots per wave for small batches
  if (batch * Hkv <= 64 && part_size <= 64 * 4 * 32)
    hipLaunchKernelGGL(paged_decode_fp8_kernel<2>, grid, dim3(256), 0, s, prm, total_items);
  else
    hipLaunchKernelGGL(paged_decode_fp8_kernel<1>, grid, dim3(256), 0, s, prm, total_items);
  return hipGetLastError();
}

}  // namespace dab
