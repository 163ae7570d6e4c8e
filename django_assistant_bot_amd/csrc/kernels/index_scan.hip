// Persistent exact-cosine scan of the in-HBM index for small query batches (M <= 96): the
// threshold-candidate pass of VectorIndex search (the pgvector CosineDistance ORDER BY it replaces:
// reference rag/services/search_service.py:185-196) at 1-96 queries.
//
// At M <= 96 the scan is an HBM stream (15 GB for 10M x 768 rows; 1 TFLOP at 64 queries, a sixth
// of the stream time on the matrix cores).  The GEMM kernels stage the queries again for every
// output tile (as many L2 bytes as the rows they scan); here they are staged into LDS ONCE per
// workgroup and every wave streams index rows through a VGPR ring for the whole launch:
//   * MT 16-query tiles (M <= 16 MT): MT 1-2 -> 4-wave workgroups, 2 per CU; MT 3-6 -> 8-wave
//     workgroups, 1 per CU (up to 144 KB of queries in LDS: MT 5-6 need K <= 768);
//   * persistent grid, tile = 32 rows per wave (two 16-row MFMA A tiles),
//     row-major 16-B loads (lane = row li, k 8g..8g+7 of a 32-k chunk) with the tile's base in the
//     buffer descriptor, whose range clamps the last partial tile to zeros;
//   * the ring runs across tile boundaries (a flat stream of 32-k chunks), so the next tile's loads
//     are in flight under the current tile's epilogue;
//   * queries [16 MT, K] in LDS with chunk c of row r at c ^ (r & 15): conflict-free ds_read_b128
//     B fragments (one fragment feeds both A tiles' MFMAs; one A fragment feeds MT MFMAs);
//   * epilogue straight from the accumulators: a score >= thr[query] (rare) takes a slot in the
//     wave's LDS list; flushing the list applies the row / query group filters and appends to the
//     query's global list with one returning atomic per hit (gemm.hip EPI_CANDIDATES) -- a wait
//     that in the tile loop would drain the wave's whole load ring;
//   * SHUF: the rows come from a copy in the decode-stream layout [rows/16][K/32][64 lanes][8]
//     (ops.shuffle_weights), where each 16-row x 32-k A fragment is 1 KB contiguous in lane order:
//     every load is one fully coalesced 1 KB read instead of 16 rows x 64 B.
//
// One kernel, index_scan_kernel<FMT, MT, NW, NWIN>, over the three row formats (ScanFmt): the
// candidate lists, the query staging, the tile walk and the hit epilogue are written once, and what
// a format changes (ring slot type and chunk width, the descriptors, the exponent loads, the MFMA
// feed, the score's scale) sits behind `if constexpr`.
//
// FP8 rows (kScanFp8, the opt-in FP8 index): the same scan over e4m3fn bytes in the
// ops.shuffle_weights_fp8 layout [rows/16][K/64][64 lanes][16 B] with one E8M0 exponent byte per row.
// A ring slot is one 16-row x 64-k fragment per A tile (16 B per lane, still one coalesced 1 KB
// read; NWIN of them in flight per wave, NWIN divides K / 64); it is converted in registers
// (fp8x8_bf16) into the two bf16 A fragments the bf16 arm would have loaded and fed to the same MFMA
// sequence in the same k order, and the row's exponent scales the fp32 sum before the threshold
// test: the scores are bit-identical to the bf16 scan over the dequantised rows.
// index_dequant_kernel turns 16-row blocks of that copy into the bf16 fragment layout for the
// callers that need a full score matrix (fp8x16_dequant, common.h).
#include <type_traits>

#include "common.h"
#include "launchers.h"

namespace dab {

namespace {

struct ScanParams {
  const bf16* X;  // queries [M, K]
  long ldx;
  const bf16* W;  // index rows [N, K]
  long ldw;
  int M, N, K;
  const int* row_group;
  const int* q_group;
  const float* thr;
  int* cnt;
  float* cand_val;
  int* cand_idx;
  int cap;
  const uint8_t* exps;  // FP8 rows: exponent byte per row (>= round_up(N, 4) of them), else unused
};

constexpr int kScanKMax = 1024;
constexpr int kScanMaxM = 96;
// widest rows the queries of MT 16-query tiles may have (LDS: 16 MT KMax 2 B <= 144 KB)
constexpr int scan_kmax(int mt) { return mt <= 4 ? kScanKMax : 768; }
constexpr int kScanRT = 2;     // 16-row A tiles per wave
constexpr int kScanNWIN = 8;   // bf16 rows: chunks (of 32 k) in flight per wave
constexpr int kScanListW = 160;  // candidate list entries per wave (12 B each)

// the rows: row-major bf16 [N, ldw]; bf16 fragments (shuffle_weights); e4m3fn fragments with one
// exponent byte per row (shuffle_weights_fp8)
enum ScanFmt { kScanRows, kScanShuf, kScanFp8 };

}  // namespace

// NWIN: ring depth in chunks (kScanNWIN for bf16 rows; FP8: divides K / 64, see index_scan_candidates_fp8)
template <ScanFmt FMT, int MT, int NW, int NWIN>
__global__ __launch_bounds__(64 * NW, 8 / NW) void index_scan_kernel(ScanParams p) {
  constexpr bool SHUF = FMT != kScanRows, FP8 = FMT == kScanFp8;
  static_assert(FP8 || NWIN == kScanNWIN, "bf16 rows: the launchers check K against a ring of kScanNWIN chunks");
  constexpr int CK = FP8 ? 64 : 32;          // k per ring chunk: 16 B per lane and A tile
  constexpr int RT = kScanRT, TR = 32 * NW;  // rows per workgroup tile
  constexpr int XS = 16 * MT * scan_kmax(MT) * 2;
  __shared__ __attribute__((aligned(16))) char xs[XS + 64 + NW * kScanListW * 12];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cpr = p.K / 8;  // 16-B chunks per query row
  const int RB = p.K * 2;

  // ---- per-wave candidate lists (after the queries): a hit takes an LDS slot; the group filters
  // and the global append (a returning atomic, whose wait would drain this wave's whole load ring)
  // run when the list is flushed -- at a high-water mark and at the end
  int* const lcnt = reinterpret_cast<int*>(xs + XS);
  int* const l_n = lcnt + 16 + w * kScanListW;
  int* const l_m = lcnt + 16 + NW * kScanListW + w * kScanListW;
  float* const l_v = reinterpret_cast<float*>(lcnt + 16 + 2 * NW * kScanListW + w * kScanListW);
  auto cand_global = [&](int m, int n, float v) {
    const int rg = p.row_group ? p.row_group[n] : 0;
    const int qgm = p.q_group ? p.q_group[m] : -1;
    if (rg >= 0 && (qgm < 0 || rg == qgm)) {
      const int slot = atomicAdd(p.cnt + m, 1);
      if (slot < p.cap) {
        p.cand_val[(size_t)m * p.cap + slot] = v;
        p.cand_idx[(size_t)m * p.cap + slot] = n;
      }
    }
  };
  auto list_count = [&]() {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(lcnt + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  };
  auto cand_flush = [&]() {  // wave-uniform
    const int c = list_count();
    for (int e = lane; e < c; e += 64) cand_global(l_m[e], l_n[e], l_v[e]);
    if (lane == 0) __hip_atomic_store(lcnt + w, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    // retire the flush's own memory ops here, so the code after it (and the hit test of every tile,
    // which the compiler merges with this path) inherits no pending store or load to wait for
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
  };
  if (tid < NW) lcnt[tid] = 0;

  // ---- queries -> LDS once (rows >= M repeat row M - 1; their scores are never appended)
  for (int e = tid; e < 16 * MT * cpr; e += 64 * NW) {
    const int r = e / cpr, c = e % cpr;
    const u32x4 v = *reinterpret_cast<const u32x4*>(p.X + (size_t)min(r, p.M - 1) * p.ldx + 8 * c);
    *reinterpret_cast<u32x4*>(xs + r * RB + 16 * (c ^ (r & 15))) = v;
  }
  float thr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + li;
    thr[t] = m < p.M ? p.thr[m] : __builtin_huge_valf();
  }
  __syncthreads();

  // ---- flat chunk stream over this wave's tiles: tile i of the wave = rows
  // (blockIdx.x + i * gridDim.x) * TR + 32 w .. + 31; chunk = CK k of both 16-row A tiles
  const int nck = p.K / CK;  // chunks per tile (a multiple of NWIN: checked by the launcher)
  const int tiles = (p.N + TR - 1) / TR;
  const int my_tiles = blockIdx.x < tiles ? (tiles - 1 - blockIdx.x) / gridDim.x + 1 : 0;
  if (my_tiles == 0) return;
  auto tile_row0 = [&](int i) { return (blockIdx.x + i * gridDim.x) * TR + 32 * w; };
  // descriptor of tile i (rows past N read zeros); past the wave's last tile or wholly past N: empty
  // range (the ring's loads return zeros without memory traffic)
  // SHUF: a chunk of a 16-row block is 1 KB in both fragment layouts ([blk][K / CK][64 lanes][16 B]);
  // a tile's two blocks are whole in the copy (round_up(N, 128) rows) when it starts below N; rows
  // >= N there score like any row and are dropped by the epilogue's n < N test
  auto rsrc_of = [&](int i) {
    const int r0 = tile_row0(i);
    const bool live = i < my_tiles && r0 < p.N;
    if constexpr (SHUF) {
      const char* const blocks = reinterpret_cast<const char*>(p.W);
      return __builtin_amdgcn_make_buffer_rsrc((void*)(blocks + (size_t)(min(r0, p.N - 1) / 16) * nck * 1024), (short)0,
                                               live ? 2 * nck * 1024 : 0, 0x00020000);
    } else {
      const int rows = live ? min(32, p.N - r0) : 0;
      return __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (size_t)min(r0, p.N - 1) * p.ldw), (short)0,
                                               (int)(rows * p.ldw * 2), 0x00020000);
    }
  };
  // FP8 (unused otherwise): the exponent bytes of rows 4 g .. + 3 of each A tile: one dword per tile
  // and lane.  Range: the whole dwords that hold a row < N (a tile past N reads zeros; its scores
  // are dropped)
  [[maybe_unused]] const auto ex_rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.exps, (short)0, (p.N + 3) / 4 * 4, 0x00020000);
  const int voff = SHUF ? lane * 16 : (int)((li * p.ldw + 8 * g) * 2);
  const int astr = SHUF ? nck * 1024 : (int)(16 * p.ldw * 2);  // next 16-row block
  constexpr int CSTR = SHUF ? 1024 : 64;                         // next chunk

  // a ring slot: one bf16 A fragment (32 k), or the 16 FP8 bytes of two (64 k)
  using slot_t = std::conditional_t<FP8, u32x4, bf16x8>;
  slot_t wr[NWIN][RT];
  [[maybe_unused]] uint32_t ex_ld[RT];  // exponents of the tile whose chunks are being loaded
  int ld_tile = 0, ld_c = 0;  // next chunk to load (wave-uniform)
  auto ld_rs = rsrc_of(0);
  auto load = [&](int slot) __attribute__((always_inline)) {
    if constexpr (FP8) {
      // slot 0 carries the exponents of its chunk's tile: no branch in the ring, and they arrive
      // with the tile's first chunk (ld_c % NWIN == slot, so chunk 0 of a tile is always slot 0's)
      if (slot == 0) {
        const int e0 = tile_row0(ld_tile) + 4 * g;
#pragma unroll
        for (int a = 0; a < RT; ++a) ex_ld[a] = __builtin_amdgcn_raw_buffer_load_b32(ex_rs, e0 + 16 * a, 0, 0);
      }
    }
#pragma unroll
    for (int a = 0; a < RT; ++a)
      wr[slot][a] = __builtin_bit_cast(
          slot_t, __builtin_amdgcn_raw_buffer_load_b128(ld_rs, voff + a * astr, ld_c * CSTR, 2));  // nt: read once
    if (++ld_c == nck) {
      ld_c = 0;
      ld_rs = rsrc_of(++ld_tile);
    }
  };
#pragma unroll
  for (int s = 0; s < NWIN; ++s) load(s);

  f32x4 acc[RT][MT];
  for (int i = 0; i < my_tiles; ++i) {
#pragma unroll
    for (int a = 0; a < RT; ++a)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] uint32_t ex[RT];  // this tile's exponents (ex_ld moves on to the next tile during the loop)
    if constexpr (FP8) {
#pragma unroll
      for (int a = 0; a < RT; ++a) ex[a] = ex_ld[a];
    }
    for (int c0 = 0; c0 < nck; c0 += NWIN) {
#pragma unroll
      for (int s = 0; s < NWIN; ++s) {
        const int c = c0 + s;
#pragma unroll
        for (int h = 0; h < CK / 32; ++h) {  // the chunk's 32-k halves (FP8: two), in k order
          bf16x8 bx[MT];
#pragma unroll
          for (int t = 0; t < MT; ++t)
            bx[t] = *reinterpret_cast<const bf16x8*>(xs + (16 * t + li) * RB + 16 * ((4 * (CK / 32 * c + h) + g) ^ li));
#pragma unroll
          for (int a = 0; a < RT; ++a) {
            bf16x8 wa;
            if constexpr (FP8) wa = fp8x8_bf16(wr[s][a][2 * h], wr[s][a][2 * h + 1]);
            else wa = wr[s][a];
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[a][t] = mfma16(wa, bx[t], acc[a][t]);
          }
        }
        load(s);  // refill the slot right behind its MFMAs (NWIN chunks ahead)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- candidates: acc[a][t] lane (li, g) = scores of query 16 t + li against rows 16 a + 4 g + r
    // (FP8: unscaled; score = acc x 2^(exponent byte - 127))
    const int r0 = tile_row0(i);
    if (r0 >= p.N) continue;  // wave-uniform
    [[maybe_unused]] float sc[RT][4];
    if constexpr (FP8) {
#pragma unroll
      for (int a = 0; a < RT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[a][r] = exp_scale((ex[a] >> (8 * r)) & 0xffu);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int a = 0; a < RT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = r0 + 16 * a + 4 * g + r;
          float v = acc[a][t][r];
          if constexpr (FP8) v *= sc[a][r];
          const bool hit = v >= thr[t] && n < p.N;
          // the list holds <= kScanListW - 64 entries here, so the <= 64 hits of one step fit
          if (__builtin_amdgcn_ballot_w64(hit)) {
            if (hit) {
              const int slot = __hip_atomic_fetch_add(lcnt + w, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              l_n[slot] = n;
              l_m[slot] = 16 * t + li;
              l_v[slot] = v;
            }
            if (list_count() > kScanListW - 64) cand_flush();
          }
        }
  }
  cand_flush();
}

// One lane per 16 B of the FP8 fragment copy: fragment [blk][j][lane] of blocks b0 .. b1 - 1 -> the
// bf16 fragments [blk - b0 + ob][2 j][lane] and [.. ][2 j + 1][lane] of `out` (shuffle_weights layout).
__global__ __launch_bounds__(256) void index_dequant_kernel(const uint8_t* __restrict__ data,
                                                            const uint8_t* __restrict__ exps, bf16* __restrict__ out,
                                                            size_t b0, size_t ob, size_t nfrag, int nck) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nfrag; i += (size_t)gridDim.x * 256) {
    const int lane = (int)(i & 63);
    const size_t f = i >> 6, blk = f / nck, j = f - blk * nck;  // blk: relative to b0
    const u32x4 d = *reinterpret_cast<const u32x4*>(data + (((b0 + blk) * nck + j) * 64 + lane) * 16);
    u32x4 o[2];
    fp8x16_dequant(d, exp_scale(exps[(b0 + blk) * 16 + (lane & 15)]), o);
    bf16* dst = out + (((ob + blk) * 2 * nck + 2 * j) * 64 + lane) * 8;
    *reinterpret_cast<u32x4*>(dst) = o[0];
    *reinterpret_cast<u32x4*>(dst + 512) = o[1];
  }
}

// exps / nwin: FP8 rows only (else nullptr / kScanNWIN)
static int index_scan_launch(ScanFmt fmt, int nwin, const void* X, long ldx, const void* W, long ldw, const void* exps,
                             int M, int N, int K, const int* row_group, const int* q_group, const float* thr, int* cnt,
                             float* cand_val, int* cand_idx, int cap, hipStream_t s) {
  ScanParams p;
  p.X = (const bf16*)X;
  p.ldx = ldx;
  p.W = (const bf16*)W;
  p.ldw = ldw;
  p.M = M;
  p.N = N;
  p.K = K;
  p.row_group = row_group;
  p.q_group = q_group;
  p.thr = thr;
  p.cnt = cnt;
  p.cand_val = cand_val;
  p.cand_idx = cand_idx;
  p.cap = cap;
  p.exps = (const uint8_t*)exps;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const int mt = (M + 15) / 16;
  const int nw = mt <= 2 ? 4 : 8, per_cu = 8 / nw;
  const long tiles = (N + 32L * nw - 1) / (32L * nw);
  const int grid = (int)(tiles < (long)per_cu * cus ? tiles : (long)per_cu * cus);
#define SCAN_KERNEL(FMT_, MT_, NW_, NWIN_) \
  hipLaunchKernelGGL((index_scan_kernel<FMT_, MT_, NW_, NWIN_>), dim3(grid), dim3(64 * NW_), 0, s, p)
#define SCAN_LAUNCH(MT_, NW_)                                                     \
  do {                                                                            \
    if (fmt == kScanRows) SCAN_KERNEL(kScanRows, MT_, NW_, kScanNWIN);            \
    else if (fmt == kScanShuf) SCAN_KERNEL(kScanShuf, MT_, NW_, kScanNWIN);       \
    else if (nwin == 8) SCAN_KERNEL(kScanFp8, MT_, NW_, 8);                       \
    else if (nwin == 6) SCAN_KERNEL(kScanFp8, MT_, NW_, 6);                       \
    else SCAN_KERNEL(kScanFp8, MT_, NW_, 4);                                      \
  } while (0)
  switch (mt) {
    case 1: SCAN_LAUNCH(1, 4); break;
    case 2: SCAN_LAUNCH(2, 4); break;
    case 3: SCAN_LAUNCH(3, 8); break;
    case 4: SCAN_LAUNCH(4, 8); break;
    case 5: SCAN_LAUNCH(5, 8); break;
    default: SCAN_LAUNCH(6, 8); break;
  }
#undef SCAN_LAUNCH
#undef SCAN_KERNEL
  return hipGetLastError();
}

int index_scan_candidates(const void* X, long ldx, const void* W, long ldw, int M, int N, int K, const int* row_group,
                          const int* q_group, const float* thr, int* cnt, float* cand_val, int* cand_idx, int cap,
                          hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (M > kScanMaxM || K > scan_kmax((M + 15) / 16) || K % (32 * kScanNWIN) || ldx % 8 || ldw % 8 || cap <= 0)
    return hipErrorInvalidValue;
  if (32L * ldw * 2 >= (1L << 31)) return hipErrorInvalidValue;
  return index_scan_launch(kScanRows, kScanNWIN, X, ldx, W, ldw, nullptr, M, N, K, row_group, q_group, thr, cnt,
                           cand_val, cand_idx, cap, s);
}

// W: the rows in the shuffle_weights layout, with at least round_up(N, 32) rows
int index_scan_candidates_shuf(const void* X, long ldx, const void* W, int M, int N, int K, const int* row_group,
                               const int* q_group, const float* thr, int* cnt, float* cand_val, int* cand_idx,
                               int cap, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (M > kScanMaxM || K > scan_kmax((M + 15) / 16) || K % (32 * kScanNWIN) || ldx % 8 || cap <= 0)
    return hipErrorInvalidValue;
  return index_scan_launch(kScanShuf, kScanNWIN, X, ldx, W, K, nullptr, M, N, K, row_group, q_group, thr, cnt,
                           cand_val, cand_idx, cap, s);
}

// W: e4m3fn bytes in the shuffle_weights_fp8 layout with at least round_up(N, 32) rows; exps: one
// exponent byte per row, 4-byte aligned, at least round_up(N, 4) of them
int index_scan_candidates_fp8(const void* X, long ldx, const void* W, const void* exps, int M, int N, int K,
                              const int* row_group, const int* q_group, const float* thr, int* cnt, float* cand_val,
                              int* cand_idx, int cap, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (M > kScanMaxM || K > scan_kmax((M + 15) / 16) || K % 256 || ldx % 8 || cap <= 0 || !exps ||
      (reinterpret_cast<uintptr_t>(exps) & 3))
    return hipErrorInvalidValue;
  // ring depth in 64-k chunks: the deepest of 8 / 6 / 4 that divides K / 64 (K % 256 == 0: 4 always does)
  const int nck = K / 64, nwin = nck % 8 == 0 ? 8 : nck % 6 == 0 ? 6 : 4;
  return index_scan_launch(kScanFp8, nwin, X, ldx, W, K, exps, M, N, K, row_group, q_group, thr, cnt, cand_val,
                           cand_idx, cap, s);
}

// 16-row blocks [b0, b1) of an FP8 fragment copy ([R, K] bytes, exps [R]) -> bf16 fragments, blocks
// [out_block, out_block + b1 - b0) of `out` (shuffle_weights layout, same K).  K % 64 == 0.
int index_dequant_blocks(const void* data, const void* exps, void* out, long b0, long b1, long out_block, int K,
                         hipStream_t s) {
  if (b1 <= b0) return 0;
  if (b0 < 0 || out_block < 0 || K <= 0 || K % 64) return hipErrorInvalidValue;
  const int nck = K / 64;
  const size_t nfrag = (size_t)(b1 - b0) * nck * 64;
  const size_t blocks = (nfrag + 255) / 256;
  hipLaunchKernelGGL(index_dequant_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s,
                     (const uint8_t*)data, (const uint8_t*)exps, (bf16*)out, (size_t)b0, (size_t)out_block, nfrag, nck);
  return hipGetLastError();
}

}  // namespace dab
