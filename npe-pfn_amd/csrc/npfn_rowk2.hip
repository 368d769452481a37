// npfn_rowk2.hip -- fused row-tile layer kernel (everything of a PerFeatureEncoderLayer but
// the item attention) with 32 token slots per wave (two 16-token blocks).
//
// Why 32 slots: with 16 tokens per wave (the r01-r03 kernel, retired in r04; git history) every
// v_mfma_f32_16x16x32_bf16 read its 1 KB weight fragment from LDS for one wave's 16 tokens, so
// the chunk loop moved 1/16 B of LDS per flop -- the whole LDS bandwidth at the MFMA peak --
// and streamed every weight chunk once per 128 tokens.  Here a wave owns 32 token slots
// (blocks b = 0, 1, slots 32w + 16b + (lane & 15)) and every weight fragment read feeds TWO
// MFMAs (one per block): half the LDS bytes per MFMA, half the LDS-DMA weight traffic and half
// the chunk barriers per token (tile = 256 slots, 8 waves).  The 16-slot kernel gave
// bit-identical results (same per-token K order; tools/bitwise_ab.py).
//
// Register budget (2 waves per SIMD, <= 256 VGPRs): the residual x (2 x 48 f32), its bf16
// B fragments xb (2 x 24) and a window of WIN weight fragments (4 each) stay
// live; the test side stores x before its item-q products (their accumulators need x's
// registers) and the train side stores q and k as soon as they are complete.
// LDS (160 KB): a 2-slot weight ring (the chunk period is twice a 16-slot kernel's, so one chunk
// of DMA lead is the same time as the 16-slot kernel's two) + the head-pair feature-attention images for 256
// slots + LayerNorm parameters (+ the encoder's tables in a layer-0 entry launch, which expands the
// tokens from k_encode_seed's 16-byte seeds instead of loading them: ENC_OFF below).
#include "npfn_common.h"
#include "npfn_kernels.h"

namespace npfn {
namespace {

constexpr int RT = 256;                              // token slots per tile (8 waves x 32)
constexpr int NSLOT = 2;                             // weight ring depth
#ifndef NPFN_ROWK_WIN
#define NPFN_ROWK_WIN 6
#endif
// weight fragments in flight per wave; r06 A/B on the current kernel: 4 +0.3 %, 8 +5.8 % (spills),
// 12 spills ~390 B (profiles/r06/ab_rowk_window_sched_r06t.txt)
constexpr int WIN = NPFN_ROWK_WIN;
static_assert(WIN >= 4 && WIN <= 12 && 24 % WIN == 0, "window: a divisor of the 24 fragments of a chunk");
constexpr int PART = 24 - WIN;                       // fragment steps before the chunk barrier
constexpr int WS_ELEMS = 192 * 64;                   // one chunk image (bf16)
constexpr int WS_BYTES = WS_ELEMS * 2;
constexpr int WS_OFF = 0;
constexpr int RTP = RT + 32;                         // value rows (+ zero pad for the last row's steps)
constexpr int RTQ = RT + 16;                         // key / query rows (+ pad for 16-row blocks)
constexpr int KH_ELEMS = RTQ * 32;                   // one head: bf16 [RTQ][32], dims in pi order
constexpr int KH_OFF = WS_OFF + NSLOT * WS_BYTES;    // keys: 2 heads
constexpr int QH_OFF = KH_OFF + 2 * KH_ELEMS * 2;    // queries: 2 heads; overwritten by the outputs
constexpr int VV_OFF = QH_OFF + 2 * KH_ELEMS * 2;    // values: bf16 [RTP][64] (the pair's dims), token-major
constexpr int FA_END = VV_OFF + RTP * 64 * 2;
constexpr int LNP_OFF = FA_END;                      // float [6][192]: ln2 g,b | ln3 g,b | ln1 g,b
constexpr int TILE_OFF = LNP_OFF + 6 * 192 * 4;      // int [2]: this / the next tile (dynamic schedule)
// Fused encoder (layer-0 entry, rows of <= 64 tokens): yencw [192][2] f32 here; encw [192][4] f32
// takes the ln2 / ln3 slots of LNP, which a launch without a post part never reads
constexpr int ENC_OFF = TILE_OFF + 16;
constexpr int SMEM_BYTES = ENC_OFF + 192 * 2 * 4;
constexpr int GLDS_PER_WAVE = 3;                     // 1 KB LDS-DMA pieces per wave per chunk
static_assert(SMEM_BYTES <= 160 * 1024, "LDS budget");

typedef f32x4 Acc[12];   // D of a 192-feature product for 16 tokens
typedef f32x4 Acc4[4];   // D of a 64-feature slab
typedef bf16x8 Frag[6];  // B operand of a K = 192 product (pi order per 32-feature step)

__device__ __forceinline__ void bar() { lds_barrier(); }
// (r05: the lane-derived LDS offsets recomputed at each use from an opaque v_mbcnt -- spills of the
// dominant instance 148 -> 72 bytes per lane -- made k_row_layer 1.3 % SLOWER, and reading the
// LayerNorm parameters from LDS at each use as well 5.7 % slower: the hoisted, spilled copies'
// reloads are hidden; profiles/r05/ab_rowk_remat_r05ae.txt)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS images of the feature attention: key / query rows of 64 B (4 units of 16 B; ds_write_b128
// by token slot, ds_read_b128 from any row start), XOR-swizzled by slot so that the writes and the
// row-relative reads are free of bank conflicts; value rows of 128 B (16 units of 8 B; ds_write_b128
// of unit pairs by token slot, ds_read_b64_tr_b16 over 8 rows x 4 units) in the r03 layout, whose
// swizzle keeps units 2k, 2k+1 adjacent.  r04 measured conflict-free layouts for the value image and
// the prefetched item-attention output as well (SQ_LDS_BANK_CONFLICT 5.1e8 -> 4e5 cycles on the
// predict workload): their index arithmetic cost more than the conflicts (c2 -0.8 % / -0.2 %,
// profiles/r04/ab_swz_r04e.txt), so only the key / query swizzle is kept.
__device__ __forceinline__ int kh_idx(int t, int u) { return t * 32 + ((u ^ ((t >> 1) & 3)) << 3); }
__device__ __forceinline__ int vv_idx(int t, int gi) { return t * 64 + ((gi ^ (((t >> 1) & 3) << 2)) << 2); }
// the next tile's item-attention output prefetched into LDS: tokens at a 384-byte stride
constexpr int kPreoStride = 192;                     // elements per token in the LDS image
constexpr int kPreoUnits = kPreoStride / 8;          // 16-byte units per token

__device__ __forceinline__ bf16x8 pack8(const f32x4& lo, const f32x4& hi) {
  uint4 u;
  u.x = pack_bf2(lo[0], lo[1]);
  u.y = pack_bf2(lo[2], lo[3]);
  u.z = pack_bf2(hi[0], hi[1]);
  u.w = pack_bf2(hi[2], hi[3]);
  return __builtin_bit_cast(bf16x8, u);
}
__device__ __forceinline__ void to_frag(const Acc& a, Frag& f) {
#pragma unroll
  for (int m = 0; m < 6; ++m) f[m] = pack8(a[2 * m], a[2 * m + 1]);
}

// 2-slot weight ring: at the barrier of chunk i (after all its fragment reads landed) chunk
// i+1 has landed for every wave, and chunk i's slot takes chunk i+2.
struct Ring {
  const char* istart;
  const char* iend;
  const char* isrc;    // next chunk to issue
  uint32_t ws_lds;     // LDS byte address of slot 0
  int slot;            // slot of the chunk being read

  __device__ __forceinline__ void issue(int dslot) {
    const int dw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t voff = (threadIdx.x & 63) * 16u;
    const uint32_t dst = ws_lds + (uint32_t)(dslot * WS_BYTES) + (uint32_t)dw * (GLDS_PER_WAVE * 1024u);
    const char* src = isrc + dw * (GLDS_PER_WAVE * 1024);
#pragma unroll
    for (int p = 0; p < GLDS_PER_WAVE; ++p) glds16_s(src + p * 1024, voff, dst + (uint32_t)p * 1024u);
    isrc += WS_BYTES;
    if (isrc == iend) isrc = istart;
  }
  __device__ __forceinline__ const bf16_t* cur(const char* smem) const {
    return reinterpret_cast<const bf16_t*>(smem + WS_OFF) + slot * WS_ELEMS;
  }
  __device__ __forceinline__ const bf16_t* advance(const char* smem) {
    wait_vmcnt<0>();  // this wave's pieces of chunk i+1 (nothing younger is in flight)
    bar();            // everyone's pieces landed, everyone's reads of chunk i landed
    issue(slot);
    slot ^= 1;
    if (tpend >= 0) {  // dynamic schedule: the next tile's index, fetched at this tile's start
      if (threadIdx.x == 0) reinterpret_cast<volatile int*>(const_cast<char*>(smem) + tslot_off)[tpend] = (int)tnext;
      tpend = -1;
    }
    return reinterpret_cast<const bf16_t*>(smem + WS_OFF) + slot * WS_ELEMS;
  }
  // dynamic tile schedule: the fetched next-tile index (lane 0 of wave 0) is written to LDS
  // slot tpend at the tile's first chunk barrier (the atomic has returned by then: vmcnt(0)),
  // so no wave waits on the atomic; the tile's later barriers publish it
  int tslot_off;
  int tpend;
  unsigned tnext;
};

enum { CK_S = 0, CK_O = 1 };
typedef bf16x8 AWin[WIN];

__device__ __forceinline__ int frag_off(int half) {
  const int lane = threadIdx.x & 63;
  return (lane & 15) * 64 + (((4 * half + (lane >> 4)) ^ (lane & 7)) << 3);
}
template <int T>
__device__ __forceinline__ bf16x8 read_frag(const bf16_t* w, int k, int o0, int o1) {
  const int e = T == CK_S ? (k % 12) * 1024 + (k >= 12 ? o1 : o0)
                          : ((k >> 2) >> 1) * 4096 + (k & 3) * 1024 + (((k >> 2) & 1) ? o1 : o0);
  return *reinterpret_cast<const bf16x8*>(w + e);
}
template <int T>
__device__ __forceinline__ void read_window(const bf16_t* w, AWin& a) {
  const int o0 = frag_off(0), o1 = frag_off(1);
#pragma unroll
  for (int k = 0; k < WIN; ++k) a[k] = read_frag<T>(w, k, o0, o1);
}

__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }
// The per-step issue pattern of a chunk (2 MFMAs, the DS read that refills the window, the step's
// share of the epilogue's VALU).  r06 A/B (profiles/r06/ab_rowk_window_sched_r06t.txt,
// ab_rowk_sched_patterns_r06u.txt): without the pattern k_row_layer is 58 % SLOWER; the DS read
// first, the VALU split around the MFMAs or the DS read between them are within +-0.3 %.
template <int N, int VALU_PER_STEP>
__device__ __forceinline__ void sched_steps() {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // the step's two MFMAs (blocks 0, 1)
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read into the freed window register
    if (VALU_PER_STEP > 0) __builtin_amdgcn_sched_group_barrier(0x002, VALU_PER_STEP, 0);
  }
}

// Chunk pipeline: fragment k of chunk i (k < 24) feeds MFMA (k, block 0) and (k, block 1) from
// window register k % WIN, which is then refilled with fragment k + WIN -- of chunk i while
// k < PART, of chunk i+1 (kind NT) after the chunk barrier.  `mma(k, frag)` issues both MFMAs.
template <int T, int NT, int VALU0, int VALU1, class MMA, class EPI>
__device__ __forceinline__ void run_chunk(Ring& ring, const char* smem, AWin& a, MMA&& mma, EPI&& epi) {
  const int o0 = frag_off(0), o1 = frag_off(1);
  const bf16_t* w = ring.cur(smem);
  sched_fence();
#pragma unroll
  for (int k = 0; k < PART; ++k) {
    mma(k, a[k % WIN]);
    a[k % WIN] = read_frag<T>(w, k + WIN, o0, o1);
  }
  epi(0);
  sched_steps<PART, VALU0>();
  sched_fence();
  const bf16_t* wn = ring.advance(smem);
#pragma unroll
  for (int k = PART; k < 24; ++k) {
    mma(k, a[k % WIN]);
    a[k % WIN] = read_frag<NT>(wn, k - PART, o0, o1);
  }
  epi(1);
  sched_steps<WIN, VALU1>();
  sched_fence();
}

// S chunk: acc[b] (+)= W X_b^T for 192 outputs over the 64-K slice whose B fragments are
// bf[b][0], bf[b][1]
template <bool INIT, int NT>
__device__ __forceinline__ void run_s(Ring& ring, const char* smem, AWin& a, const bf16x8 (&bf)[2][2], Acc (&acc)[2]) {
  run_chunk<CK_S, NT, 0, 0>(
      ring, smem, a,
      [&](int k, const bf16x8& fr) {
        const int f = k % 12;
        const bool first = k < 12;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const f32x4 c = (INIT && first) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[b][f];
          acc[b][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr, bf[b][first ? 0 : 1], c, 0, 0, 0);
        }
      },
      [](int) {});
}

// O chunk: acc[b] = W_s X_b^T for a 64-output slab over all of K = 192
template <int NT>
__device__ __forceinline__ void run_o(Ring& ring, const char* smem, AWin& a, const Frag (&xb)[2], Acc4 (&acc)[2]) {
  run_chunk<CK_O, NT, 0, 0>(
      ring, smem, a,
      [&](int k, const bf16x8& fr) {
        const int ks = k >> 2, f = k & 3;
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[b][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr, xb[b][ks],
                                                              ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[b][f], 0, 0, 0);
      },
      [](int) {});
}

// GELU of a D tile.  (r05: the same arithmetic on feature pairs -- v_pk_mul / v_pk_fma /
// v_pk_add_f32 beside the per-value exp2 and rcp, 18 instead of 28 VALU per tile, bitwise equal
// -- made k_row_layer 0.9 % SLOWER, as r03's attempt was not faster: the W2 chunks that carry the
// GELU are not bound by its issue count; profiles/r05/ab_tgt_pkgelu_r05k.txt)
__device__ __forceinline__ void gelu4(f32x4& h) {
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = gelu_tanh(h[r]);
}

// GELU tiles (b, f) = t >> 2, t & 3 of the 8 slab tiles: the first NG0 in the part before the
// chunk barrier, the rest after it (about the parts' MFMA shares)
constexpr int NG0 = (8 * PART + 12) / 24;

// S chunk of W2 slab s-1 (x += h_{s-1} W2[:, s-1]^T) with the GELU of slab s in its shadow;
// n[b][0..1] = GELU(h_s) as W2's B fragments of slab s
template <int NT>
__device__ __forceinline__ void run_w2_gelu(Ring& ring, const char* smem, AWin& a, const bf16x8 (&hp)[2][2],
                                            Acc (&x)[2], Acc4 (&h)[2], bf16x8 (&n)[2][2]) {
  run_chunk<CK_S, NT, (NG0 * 28 + PART - 1) / PART, ((8 - NG0) * 28 + 8 + WIN - 1) / WIN>(
      ring, smem, a,
      [&](int k, const bf16x8& fr) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
          x[b][k % 12] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr, hp[b][k < 12 ? 0 : 1], x[b][k % 12], 0, 0, 0);
      },
      [&](int part) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
          if ((part == 0) == (t < NG0)) gelu4(h[t >> 2][t & 3]);
        if (part == 1) {
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            n[b][0] = pack8(h[b][0], h[b][1]);
            n[b][1] = pack8(h[b][2], h[b][3]);
          }
        }
      });
}

// x = LN(x) * gamma + beta over the token's 192 features (lanes l, l^16, l^32, l^48), one pass:
// the sum and the sum of squares together (var = E[x^2] - mean^2 in f32: the post-norm
// residual's mean is O(1) against its spread, the cancellation costs ~1e-7 relative; the
// two-pass form of the retired 16-slot kernel differed in the last bits, tests/test_gpu_*.py hold both to the
// oracle).  Statistics and normalisation are split so the statistics can accumulate inside the
// last product of the sub-layer and the normalisation inside the next one (ln_stats_tile,
// ln_coef, ln_norm_tile); layer_norm is the three in a row.
struct LnStats {
  float s[2][4], q[2][4];
};
__device__ __forceinline__ void ln_stats_zero(LnStats& st) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) st.s[b][r] = st.q[b][r] = 0.f;
}
__device__ __forceinline__ void ln_stats_tile(LnStats& st, int b, const f32x4& t) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    st.s[b][r] += t[r];
    st.q[b][r] = fmaf(t[r], t[r], st.q[b][r]);
  }
}
struct LnCoef {
  float rstd, nmr;
};
__device__ __forceinline__ LnCoef ln_coef(const LnStats& st, int b) {
  float s = (st.s[b][0] + st.s[b][1]) + (st.s[b][2] + st.s[b][3]);
  float q = (st.q[b][0] + st.q[b][1]) + (st.q[b][2] + st.q[b][3]);
  s = xor32_sum(xor16_sum(s));
  q = xor32_sum(xor16_sum(q));
  const float mean = s * (1.0f / 192.0f);
  const float var = fmaxf(fmaf(-mean, mean, q * (1.0f / 192.0f)), 0.f);
  const float rstd = 1.0f / sqrtf(var + 1e-5f);
  return LnCoef{rstd, -mean * rstd};
}
__device__ __forceinline__ void ln_norm_tile(f32x4& t, int f, const LnCoef& c, const float* lnp) {
  const int g4 = (threadIdx.x & 63) >> 4;
  const f32x4 gg = *reinterpret_cast<const f32x4*>(lnp + f * 16 + g4 * 4);
  const f32x4 bb = *reinterpret_cast<const f32x4*>(lnp + 192 + f * 16 + g4 * 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) t[r] = fmaf(fmaf(t[r], c.rstd, c.nmr), gg[r], bb[r]);
}
__device__ __forceinline__ void layer_norm(Acc& x, const float* lnp) {
  LnStats st;
  ln_stats_zero(st);
#pragma unroll
  for (int f = 0; f < 12; ++f) ln_stats_tile(st, 0, x[f]);
  const LnCoef c = ln_coef(st, 0);
#pragma unroll
  for (int f = 0; f < 12; ++f) ln_norm_tile(x[f], f, c, lnp);
}
__device__ __forceinline__ void ln_frag(Acc (&x)[2], Frag (&xb)[2], const float* lnp) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    layer_norm(x[b], lnp);
    to_frag(x[b], xb[b]);
  }
}


typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ bf16x8 read_vt(const char* smem, int k0, int gi0) {
  const int lane = threadIdx.x & 63, g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const bf16_t* vv = reinterpret_cast<const bf16_t*>(smem + VV_OFF) + vv_idx(k0 + 4 * g + q, gi0 + p);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)vv);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(vv + 16 * 64));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// Row-relative feature attention of one head pair over the tile's rows: (row, head,
// 16-query block) items over the 8 waves, one item per wave at a time.
// Measured r06, code in git history: a reference-free form (P = exp2(s) without the row max, the
// exact form only for an item whose sums leave [2^-60, 2^60]) made k_row_layer -0.2 to -0.5 % in
// three same-GPU A/Bs (profiles/r06/ab_fa_nomax_r06a.txt, ab_fa_ilp_r06c.txt, ab_gelu16_r06g.txt),
// but its changed rounding moved tests/test_gpu_engine.py::test_item_attn_score_scale_stress past
// its x16 margin (fast-pass TV to the fp32 oracle 0.0498 vs the online pass's 0.0441 + 0.005;
// profiles/r06/gputests_suite_fanomax_r06o.txt), so the exact form stayed.  Two interleaved items
// per wave were 2.4 % SLOWER alone and 9 % with the no-max form (the extra live registers
// spilled; ab_fa_ilp_r06c.txt).
template <int NKB>
__device__ __forceinline__ void feat_attn_rows_t(char* smem, int C, int nrows) {
  constexpr int nkb = NKB, nst = (NKB + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, g4 = lane >> 4;
  const int items = nrows * 2 * nkb;
  const int lim0 = C - 4 * g4;
  for (int it = wave; it < items; it += 8) {
    const int rh = it / nkb, qb = it - rh * nkb, r = rh >> 1;
    const int hh = rh & 1;
    const int rs = r * C, re = rs + C;
    const bf16_t* kh = reinterpret_cast<const bf16_t*>(smem + KH_OFF) + hh * KH_ELEMS;
    bf16_t* qh = reinterpret_cast<bf16_t*>(smem + QH_OFF) + hh * KH_ELEMS;
    const int qt = rs + 16 * qb + col;
    const bf16x8 qf = *reinterpret_cast<const bf16x8*>(qh + kh_idx(qt, g4));
    const bf16_t* kp = kh + kh_idx(rs + col, g4);
    f32x4 sc[4];
    float l;
    // the row max subtracted before exp2 (the sum in key order, no 0 + first).  A lambda called
    // once on purpose: written inline the compiler orders the item's instructions differently,
    // and the kernel is held to the measured build's instructions (tools/asm_cmp.py)
    auto exact = [&]() {
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        if (kb < nkb) {
          const bf16x8 ak = *reinterpret_cast<const bf16x8*>(kp + kb * 16 * 32);
          sc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          const int lim = lim0 - 16 * kb;
#pragma unroll
          for (int i = 0; i < 4; ++i) sc[kb][i] = i < lim ? sc[kb][i] : -INFINITY;
          mx = max3f(mx, sc[kb][0], sc[kb][1]);
          mx = max3f(mx, sc[kb][2], sc[kb][3]);
        } else {
          sc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      mx = xor32_max(xor16_max(mx));
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        if (kb < nkb) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[kb][i] = __builtin_amdgcn_exp2f(sc[kb][i] - mx);
            l = (kb == 0 && i == 0) ? sc[0][0] : l + sc[kb][i];
          }
        }
      }
      l = xor32_sum(xor16_sum(l));
    };
    exact();
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      if (st < nst) {
        const bf16x8 bp = pack8(sc[2 * st], sc[2 * st + 1]);
#pragma unroll
        for (int d = 0; d < 2; ++d)
          o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_vt(smem, rs + 32 * st, 8 * hh + 4 * d), bp, o[d], 0, 0, 0);
      }
    }
    const float inv = __builtin_amdgcn_rcpf(l);
    if (qt < re) *reinterpret_cast<bf16x8*>(qh + kh_idx(qt, g4)) = pack8(o[0] * inv, o[1] * inv);
  }
}

// Rows of more than 64 tokens (tabpfn-sized tables: C <= 256, one row per tile above 128):
// the same items, scores, masks, row max, key-order sum and P V products as
// feat_attn_rows_t, in two passes over the row's 16-key blocks -- the exact row max first
// (QK^T once per block), then per 32-key step the scores again, exp2, the sum and the P V
// MFMAs -- so the register footprint does not grow with C (run with C <= 64 it gives
// feat_attn_rows_t's results bit for bit).
__device__ __forceinline__ void feat_attn_rows_long(char* smem, int C, int nrows) {
  const int nkb = (C + 15) >> 4, nst = (nkb + 1) >> 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, g4 = lane >> 4;
  const int items = nrows * 2 * nkb;
  for (int it = wave; it < items; it += 8) {
    const int rh = it / nkb, qb = it - rh * nkb, h = rh & 1, r = rh >> 1;
    const int rs = r * C, re = rs + C;
    const bf16_t* kh = reinterpret_cast<const bf16_t*>(smem + KH_OFF) + h * KH_ELEMS;
    bf16_t* qh = reinterpret_cast<bf16_t*>(smem + QH_OFF) + h * KH_ELEMS;
    const int qt = rs + 16 * qb + col;
    const bf16x8 qf = *reinterpret_cast<const bf16x8*>(qh + kh_idx(qt, g4));
    const bf16_t* kp = kh + kh_idx(rs + col, g4);
    const int lim0 = C - 4 * g4;
    auto scores = [&](int kb) -> f32x4 {
      const bf16x8 ak = *reinterpret_cast<const bf16x8*>(kp + kb * 16 * 32);
      f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      const int lim = lim0 - 16 * kb;
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = i < lim ? s[i] : -INFINITY;
      return s;
    };
    float mx = -INFINITY;
    for (int kb = 0; kb < nkb; ++kb) {
      const f32x4 s = scores(kb);
      mx = max3f(mx, s[0], s[1]);
      mx = max3f(mx, s[2], s[3]);
    }
    mx = xor32_max(xor16_max(mx));
    float l = 0.f;
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int st = 0; st < nst; ++st) {
      f32x4 sc[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kb = 2 * st + u;
        if (kb < nkb) {
          sc[u] = scores(kb);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[u][i] = __builtin_amdgcn_exp2f(sc[u][i] - mx);
            l = (kb == 0 && i == 0) ? sc[0][0] : l + sc[u][i];  // key order, no 0 + first
          }
        } else {
          sc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      const bf16x8 bp = pack8(sc[0], sc[1]);
#pragma unroll
      for (int d = 0; d < 2; ++d)
        o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_vt(smem, rs + 32 * st, 8 * h + 4 * d), bp, o[d], 0, 0, 0);
    }
    l = xor32_sum(xor16_sum(l));
    const float inv = __builtin_amdgcn_rcpf(l);
    if (qt < re) *reinterpret_cast<bf16x8*>(qh + kh_idx(qt, g4)) = pack8(o[0] * inv, o[1] * inv);
  }
}

// LONG: the launch holds rows of more than 64 tokens (a separate kernel instance, so the
// common instances carry no code or registers of the long-row form)
template <bool LONG>
__device__ __forceinline__ void feat_attn_rows(char* smem, int C, int nrows) {
  if constexpr (LONG) {
    if (C > 64) {
      feat_attn_rows_long(smem, C, nrows);
      return;
    }
  }
  switch ((C + 15) >> 4) {
    case 1: feat_attn_rows_t<1>(smem, C, nrows); break;
    case 2: feat_attn_rows_t<2>(smem, C, nrows); break;
    case 3: feat_attn_rows_t<3>(smem, C, nrows); break;
    default: feat_attn_rows_t<4>(smem, C, nrows); break;
  }
}

// a token's 192 features from the D tiles (features 16f + 4 g4 + i): base (uniform) + off
// (the lane's token row start + 4 g4, in elements).  v_permlane16_swap pairs the half rows
// g4 = 0|1 and 2|3 of two feature blocks, so each lane stores 16 contiguous bytes per block pair
// (6 instead of 12 stores; r04: k_row_layer -1.4 %, bitwise equal)
__device__ __forceinline__ void store_bf16_row(bf16_t* base, int off, const Acc& a) {
  // after the swaps an even half row holds features 16f + 4g4 + [0, 8) of block f, an odd one
  // features 16(f+1) + 4(g4-1) + [0, 8) of block f+1: 16f + 4g4 + 12 from its own row start
  const int odd = (threadIdx.x >> 4) & 1;
  bf16_t* p = base + off + odd * 12;
#pragma unroll
  for (int f = 0; f < 12; f += 2) {
    uint32_t a0 = pack_bf2(a[f][0], a[f][1]), a1 = pack_bf2(a[f][2], a[f][3]);
    uint32_t b0 = pack_bf2(a[f + 1][0], a[f + 1][1]), b1 = pack_bf2(a[f + 1][2], a[f + 1][3]);
    const auto r0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
    *reinterpret_cast<uint4*>(p + f * 16) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
  }
}
__device__ __forceinline__ void store_f32_row(float* base, int off, const Acc& a) {
#pragma unroll
  for (int f = 0; f < 12; ++f) *reinterpret_cast<f32x4*>(base + off + f * 16) = a[f];
}

// One head pair of the pre phase: v, k, q O chunks into the LDS
// images, the row-relative attention, x += o_hp Wo_f[:, hp]^T (S chunk followed by kind NT)
template <int NT, bool LONG>
__device__ __forceinline__ void feat_pair(Ring& ring, char* smem, AWin& a, const Frag (&xb)[2], Acc (&x)[2],
                                          const int (&th)[2], const bool (&tv)[2], int C, int nrows) {
  const int g4 = (threadIdx.x & 63) >> 4;
  Acc4 kq[2];
  run_o<CK_O>(ring, smem, a, xb, kq);  // values of heads 2hp, 2hp+1: dims 16f + 4g4 + i
  {
    bf16_t* vv = reinterpret_cast<bf16_t*>(smem + VV_OFF);
    // the store_bf16_row pairing: an even half row writes units 4f + g4, +1 of block f, an odd
    // one units 4(f+1) + g4 - 1, +1 of block f+1 -- adjacent and 16-byte aligned in vv_idx
    const int godd = g4 & 1;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int f = 0; f < 4; f += 2) {
        const uint32_t a0 = pack_bf2(kq[b][f][0], kq[b][f][1]), a1 = pack_bf2(kq[b][f][2], kq[b][f][3]);
        const uint32_t b0 = pack_bf2(kq[b][f + 1][0], kq[b][f + 1][1]), b1 = pack_bf2(kq[b][f + 1][2], kq[b][f + 1][3]);
        const auto r0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
        const auto r1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
        *reinterpret_cast<uint4*>(vv + vv_idx(th[b], 4 * f + g4 + 3 * godd)) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
      }
  }
  run_o<CK_O>(ring, smem, a, xb, kq);  // keys
  {
    bf16_t* kh = reinterpret_cast<bf16_t*>(smem + KH_OFF);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      *reinterpret_cast<bf16x8*>(kh + kh_idx(th[b], g4)) = pack8(kq[b][0], kq[b][1]);
      *reinterpret_cast<bf16x8*>(kh + KH_ELEMS + kh_idx(th[b], g4)) = pack8(kq[b][2], kq[b][3]);
    }
  }
  run_o<CK_S>(ring, smem, a, xb, kq);  // queries (weights carry 1/sqrt(32) log2 e)
  {
    bf16_t* qh = reinterpret_cast<bf16_t*>(smem + QH_OFF);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      *reinterpret_cast<bf16x8*>(qh + kh_idx(th[b], g4)) = pack8(kq[b][0], kq[b][1]);
      *reinterpret_cast<bf16x8*>(qh + KH_ELEMS + kh_idx(th[b], g4)) = pack8(kq[b][2], kq[b][3]);
    }
  }
  bar();  // every wave's v, k, q of the pair in LDS
  feat_attn_rows<LONG>(smem, C, nrows);
  bar();  // every item's output in the query image
  bf16x8 of[2][2];
  {
    const bf16_t* qh = reinterpret_cast<const bf16_t*>(smem + QH_OFF);
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        of[b][j] = tv[b] ? *reinterpret_cast<const bf16x8*>(qh + j * KH_ELEMS + kh_idx(th[b], g4)) : bf16x8{};
  }
  run_s<false, NT>(ring, smem, a, of, x);  // x += o_hp Wo_f[:, hp]^T
}

}  // namespace

// At the end of a tile with a pre part, the next tile's item-attention output (<= 256 tokens x
// 384 B) is DMA'd into the feature-attention images (free from the last head pair's output read
// until the next tile's first head pair), so the next tile's first products read it from LDS
// instead of waiting for HBM (r03: -1.9 % kernel time)
static_assert(((RT * kPreoUnits + 511) / 512) * 8 * 1024 <= FA_END - KH_OFF,
              "the next tile's o fits the feature-attention images");

template <bool TRAIN, bool POST, bool PRE, bool LONG>
__device__ __forceinline__ void row_layer_body(const RowLayerParams& P, char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g4 = lane >> 4;
  const int th[2] = {wave * 32 + col, wave * 32 + 16 + col};  // this lane's token slots
  const int nslab = P.dff / 64;
  const int64_t ntiles = P.ntiles;
  if ((int64_t)blockIdx.x >= ntiles) return;
  const char* stream = reinterpret_cast<const char*>(P.stream);
  Ring ring{stream, stream + (int64_t)P.stream_chunks * WS_BYTES, stream, (uint32_t)(uintptr_t)(smem + WS_OFF), 0,
            TILE_OFF, -1, 0u};
  const float* lnp = reinterpret_cast<const float*>(smem + LNP_OFF);

  // the layer-0 entry expands the tokens from their seeds (encode_seed / encode_expand of
  // npfn_kernels.hip) instead of reading them from resid
  constexpr bool ENC = !POST && !LONG;
  const bool enc = ENC && P.encw != nullptr;
  ring.issue(0);
  ring.issue(1);
  if (tid < 288) {
    const int a = tid / 48, o = (tid - a * 48) * 4;
    const float* src = a == 0 ? P.ln2g : a == 1 ? P.ln2b : a == 2 ? P.ln3g : a == 3 ? P.ln3b : a == 4 ? P.ln1g : P.ln1b;
    if (enc && a < 4) src = P.encw + a * 192;  // floats [4 tid, 4 tid + 4): encw row tid
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (src) v = *reinterpret_cast<const f32x4*>(src + o);
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(smem + LNP_OFF) + a * 192 + o) = v;
  } else if (enc && tid < 288 + 96) {
    const int o = (tid - 288) * 4;
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(smem + ENC_OFF) + o) = *reinterpret_cast<const f32x4*>(P.yencw + o);
  }
  for (int i = tid; i < (FA_END - KH_OFF) / 16; i += 512)
    *reinterpret_cast<uint4*>(smem + KH_OFF + 16 * i) = make_uint4(0, 0, 0, 0);
  // Tile schedule.  Dynamic (P.tile_ctr): lane 0 of wave 0 fetches the next tile from the
  // stream's counter at the start of each tile and writes it to the LDS slot the other waves
  // read at the next tile's start (the tile's chunk barriers lie between), so a workgroup that
  // started late -- its CU busy with a side-stream kernel -- or runs slow takes fewer tiles
  // instead of holding up the launch's end.  Static: tiles blockIdx.x, + gridDim.x, ...
  // Which workgroup runs a tile does not change its arithmetic.
  const bool dyn = P.tile_ctr != nullptr;
  volatile int* const tslot = reinterpret_cast<volatile int*>(smem + TILE_OFF);
  // tiles are the counter's unsigned distance from the launch's base: a counter that drifted
  // from the host's base (a failed launch, a reused stream) reads as a huge tile and ends the
  // loop instead of indexing below the first tile
  if (dyn && tid == 0) tslot[0] = (int)(atomicAdd(P.tile_ctr, 1u) - P.tile_base);
  constexpr int FIRST = POST ? CK_S : CK_O;
  AWin a;
  wait_vmcnt<GLDS_PER_WAVE>();  // chunk 0 (chunk 1 stays in flight)
  bar();
  read_window<FIRST>(reinterpret_cast<const bf16_t*>(smem + WS_OFF), a);
  int par = 0;
  bool o_in_lds = false;  // this tile's item-attention output was prefetched into LDS
  for (int64_t tile = dyn ? (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane(tslot[0]) : (int64_t)blockIdx.x;
       tile < ntiles;
       tile = dyn ? (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane(tslot[par]) : tile + gridDim.x) {
    if (dyn) {
      par ^= 1;
      if (tid == 0) ring.tnext = atomicAdd(P.tile_ctr, 1u) - P.tile_base;
      ring.tpend = par;
    }
    RowSeg sg = P.seg[0];
#pragma unroll
    for (int i = 1; i < kRowSegs; ++i)
      if (i < P.nseg && tile >= P.seg[i].tile0) sg = P.seg[i];
    const int C = sg.C;
    const int64_t tpe = (P.R + sg.rpt - 1) / sg.rpt;
    const int64_t lt = tile - sg.tile0;
    const int64_t te = lt / tpe;
    const int64_t rt = (lt - te * tpe) * sg.rpt;
    const int64_t row0 = te * P.R + rt;
    const int nrows = (int)max((int64_t)0, min((int64_t)sg.rpt, P.R - rt));
    const bool tv[2] = {th[0] < nrows * C, th[1] < nrows * C};
    // the slots whose rows (residual, item projections) are stored: every valid one, or with
    // P.tgt_only (the last layer's pre part) the rows' target tokens only
    const bool sv[2] = {tv[0] && (!P.tgt_only || th[0] % C == C - 1), tv[1] && (!P.tgt_only || th[1] % C == C - 1)};
    // uniform tile bases + 32-bit per-lane offsets (no 64-bit per-lane addresses to keep live);
    // the post-only last layer runs the rows' target tokens (RowSeg tmem / tofs / tstride)
    const int64_t tok0 = PRE ? row0 * C : row0 * sg.tmem + sg.tofs;
    const int tsl = PRE ? 192 : sg.tstride * 192;
    float* const rbase = sg.resid + tok0 * 192;
    const int to[2] = {th[0] * tsl + g4 * 4, th[1] * tsl + g4 * 4};  // the lane's token rows
    // a slot past the tile's rows loads the tile's first token instead (finite values, never
    // stored; its keys are masked and its values meet zero probabilities in the attention), so
    // the loads need no per-slot branches
    const int lo[2] = {tv[0] ? to[0] : g4 * 4, tv[1] ? to[1] : g4 * 4};
    Acc x[2];
    if (ENC && enc) {
      // x[b][f][i] = feature 16f + 4g4 + i of the slot's token by k_encode's encode_expand (bit for
      // bit its tokens), x holding the positional value first; the positional row comes from global memory (C x 768 B, cache-resident)
      // (the lane's quarter through an opaque move: its table offsets are then computed here, once
      // per tile, instead of being hoisted into registers that stay live -- and spill -- all kernel)
      int g4e;
      asm volatile("v_mov_b32 %0, %1" : "=v"(g4e) : "v"(g4));
      const float* ew = reinterpret_cast<const float*>(smem + LNP_OFF) + g4e * 16;
      const float* yw = reinterpret_cast<const float*>(smem + ENC_OFF) + g4e * 8;
      const float* const seedb = sg.seed + tok0 * 4;  // uniform bases + 32-bit lane offsets, as below
      f32x4 sa[2];
      bool tg[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int t = tv[b] ? th[b] : 0;
        const int c = t % C;
        tg[b] = c == sg.G;
        sa[b] = *reinterpret_cast<const f32x4*>(seedb + t * 4);
        const int po = (tg[b] ? 0 : c) * 192 + g4e * 4;
#pragma unroll
        for (int f = 0; f < 12; ++f) x[b][f] = *reinterpret_cast<const f32x4*>(P.pos + po + f * 16);
      }
#pragma unroll
      for (int f = 0; f < 12; ++f) {
        const f32x4 y01 = *reinterpret_cast<const f32x4*>(yw + f * 32);
        const f32x4 y23 = *reinterpret_cast<const f32x4*>(yw + f * 32 + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(ew + f * 64 + i * 4);
          const float y0 = i < 2 ? y01[2 * i] : y23[2 * i - 4], y1 = i < 2 ? y01[2 * i + 1] : y23[2 * i - 3];
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            x[b][f][i] = encode_expand(tg[b], tg[b] ? y0 : w[0], tg[b] ? y1 : w[1], w[2], w[3], x[b][f][i], sa[b][0],
                                       sa[b][1], sa[b][2], sa[b][3]);
          }
        }
        sched_fence();  // one feature block's weights live at a time (the max-ILP scheduler hoists every read)
      }
    } else {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int f = 0; f < 12; ++f) x[b][f] = *reinterpret_cast<const f32x4*>(rbase + lo[b] + f * 16);
    }

    Frag xb[2];
    if constexpr (POST) {
      {
        bf16x8 ob[2][6];  // item-attention output in pi order
        const bf16_t* obase = sg.o_item + tok0 * 192;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int m = 0; m < 6; ++m) {
            uint2 l2, h2;
            if (PRE && o_in_lds) {  // the LDS image (kPreoStride)
              const bf16_t* ol = reinterpret_cast<const bf16_t*>(smem + KH_OFF) + (tv[b] ? th[b] : 0) * kPreoStride;
              l2 = *reinterpret_cast<const uint2*>(ol + g4 * 4 + 32 * m);
              h2 = *reinterpret_cast<const uint2*>(ol + g4 * 4 + 32 * m + 16);
            } else {
              l2 = *reinterpret_cast<const uint2*>(obase + lo[b] + 32 * m);
              h2 = *reinterpret_cast<const uint2*>(obase + lo[b] + 32 * m + 16);
            }
            ob[b][m] = __builtin_bit_cast(bf16x8, make_uint4(l2.x, l2.y, h2.x, h2.y));
          }
#pragma unroll
        for (int kc = 0; kc < 3; ++kc) {  // x += o_item Wo_i^T
          const bf16x8 bf[2][2] = {{ob[0][2 * kc], ob[0][2 * kc + 1]}, {ob[1][2 * kc], ob[1][2 * kc + 1]}};
          if (kc < 2) run_s<false, CK_S>(ring, smem, a, bf, x);
          else run_s<false, CK_O>(ring, smem, a, bf, x);
        }
      }
      ln_frag(x, xb, lnp + 0 * 384);
      // MLP, software-pipelined over 64-wide hidden slabs: W1_0 | W1_1, W2_0 (+GELU 1) | ...
      Acc4 h[2];
      bf16x8 hp[2][2];  // GELU(h_{s-1}) as W2's B fragments
      run_o<CK_O>(ring, smem, a, xb, h);
#pragma unroll
      for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int f = 0; f < 4; ++f) gelu4(h[b][f]);
        hp[b][0] = pack8(h[b][0], h[b][1]);
        hp[b][1] = pack8(h[b][2], h[b][3]);
      }
#pragma unroll 1
      for (int s = 1; s < nslab - 1; ++s) {
        run_o<CK_S>(ring, smem, a, xb, h);  // h_s = x W1_s^T
        bf16x8 hn[2][2];
        run_w2_gelu<CK_O>(ring, smem, a, hp, x, h, hn);  // x += GELU(h_{s-1}) W2_{s-1}^T; GELU(h_s)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          hp[b][0] = hn[b][0];
          hp[b][1] = hn[b][1];
        }
      }
      {
        run_o<CK_S>(ring, smem, a, xb, h);  // the last slab
        bf16x8 hn[2][2];
        run_w2_gelu<CK_S>(ring, smem, a, hp, x, h, hn);
        run_s<false, PRE ? CK_O : FIRST>(ring, smem, a, hn, x);  // x += GELU(h_last) W2_last^T
      }
      ln_frag(x, xb, lnp + 1 * 384);
      if constexpr (!PRE) {  // last layer: bf16 x of the target tokens, packed by row, for the decoder
#pragma unroll
        for (int b = 0; b < 2; ++b)
          if (tv[b]) store_bf16_row(sg.out + row0 * 192, th[b] * 192 + g4 * 4, x[b]);
        continue;
      }
    } else {
#pragma unroll
      for (int b = 0; b < 2; ++b) to_frag(x[b], xb[b]);
    }

    // ---- pre of the next layer: head pairs (the first one's v chunk finishing LN3 after a post
    // part); Wo_f's slice of the last pair is followed by the item q chunk (S)
#pragma unroll 1
    for (int hp_i = 0; hp_i < 2; ++hp_i) feat_pair<CK_O, LONG>(ring, smem, a, xb, x, th, tv, C, nrows);
    feat_pair<CK_S, LONG>(ring, smem, a, xb, x, th, tv, C, nrows);
    if constexpr (POST && PRE) {
      // every wave's reads of the images ended before feat_pair's chunk barrier; the DMA lands
      // before the next tile's start (the item-q chunks' vmcnt(0) waits and barriers)
      const int64_t nt = dyn ? (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane(tslot[par]) : tile + gridDim.x;
      o_in_lds = nt < ntiles;
      if (o_in_lds) {
        RowSeg sn = P.seg[0];
#pragma unroll
        for (int i = 1; i < kRowSegs; ++i)
          if (i < P.nseg && nt >= P.seg[i].tile0) sn = P.seg[i];
        const int64_t tpn = (P.R + sn.rpt - 1) / sn.rpt;
        const int64_t ln_ = nt - sn.tile0;
        const int64_t ten = ln_ / tpn;
        const int64_t rtn = (ln_ - ten * tpn) * sn.rpt;
        const int nrn = (int)max((int64_t)0, min((int64_t)sn.rpt, P.R - rtn));
        const int ntok = nrn * sn.C;
        const bf16_t* src = sn.o_item + (ten * P.R + rtn) * sn.C * 192;
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        constexpr int kPieces = (RT * kPreoUnits + 8 * 64 - 1) / (8 * 64);  // 1 KB pieces per wave
#pragma unroll
        for (int p = 0; p < kPieces; ++p) {
          // LDS unit L = this lane's 16 B of the piece: token L / 25, unit L % 25 (the pad unit
          // takes a copy of unit 0)
          const int piece = wv * kPieces + p;
          const int L = piece * 64 + lane, t = L / kPreoUnits, u = L - t * kPreoUnits;
          if (t < ntok)
            glds16_s(src, (uint32_t)(t * 384 + (u < 24 ? u : 0) * 16),  // (24 units: no pad)
                     (uint32_t)(uintptr_t)(smem + KH_OFF) + (uint32_t)piece * 1024u);
        }
      }
    }
    ln_frag(x, xb, lnp + 2 * 384);
    // x is final: store it, its registers then hold the item projections' accumulators
#pragma unroll
    for (int b = 0; b < 2; ++b)
      if (sv[b]) store_f32_row(rbase, to[b], x[b]);
    const bf16x8 k0[2][2] = {{xb[0][0], xb[0][1]}, {xb[1][0], xb[1][1]}};
    const bf16x8 k1[2][2] = {{xb[0][2], xb[0][3]}, {xb[1][2], xb[1][3]}};
    const bf16x8 k2[2][2] = {{xb[0][4], xb[0][5]}, {xb[1][4], xb[1][5]}};
    run_s<true, CK_S>(ring, smem, a, k0, x);  // item-attention q
    run_s<false, CK_S>(ring, smem, a, k1, x);
    if constexpr (!TRAIN) {
      run_s<false, FIRST>(ring, smem, a, k2, x);  // next: the next tile's first chunk
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if (sv[b]) store_bf16_row(sg.out + tok0 * 192, to[b], x[b]);
      continue;
    }
    // train side: q | k | v rows of width 576, each stored as soon as it is complete
    run_s<false, CK_S>(ring, smem, a, k2, x);
#pragma unroll
    for (int b = 0; b < 2; ++b)
      if (sv[b]) store_bf16_row(sg.out + tok0 * 576, 3 * to[b] - 2 * g4 * 4 + 0, x[b]);
    run_s<true, CK_S>(ring, smem, a, k0, x);  // item-attention k
    run_s<false, CK_S>(ring, smem, a, k1, x);
    run_s<false, CK_S>(ring, smem, a, k2, x);
#pragma unroll
    for (int b = 0; b < 2; ++b)
      if (sv[b]) store_bf16_row(sg.out + tok0 * 576, 3 * to[b] - 2 * g4 * 4 + 192, x[b]);
    run_s<true, CK_S>(ring, smem, a, k0, x);  // item-attention v
    run_s<false, CK_S>(ring, smem, a, k1, x);
    run_s<false, FIRST>(ring, smem, a, k2, x);  // next: the next tile's first chunk
#pragma unroll
    for (int b = 0; b < 2; ++b)
      if (sv[b]) store_bf16_row(sg.out + tok0 * 576, 3 * to[b] - 2 * g4 * 4 + 384, x[b]);
  }  // tiles
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the wrapped-around DMA
}

template <bool TRAIN, bool POST, bool PRE, bool LONG>
// (r05: a static s_setprio 1 for waves 4-7 -- the guide's "younger half" -- or for waves 0-3 was
// within noise, -0.3 / -0.2 % on c2; profiles/r05/ab_rowk_prio_r05z.txt)
__global__ __launch_bounds__(512, 1) void k_row_layer(RowLayerParams P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  row_layer_body<TRAIN, POST, PRE, LONG>(P, smem);
}

template <bool LONG>
static void rowk_setup_t() {
  (void)hipFuncSetAttribute((const void*)k_row_layer<false, false, true, LONG>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
  (void)hipFuncSetAttribute((const void*)k_row_layer<false, true, true, LONG>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
  (void)hipFuncSetAttribute((const void*)k_row_layer<false, true, false, LONG>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
  (void)hipFuncSetAttribute((const void*)k_row_layer<true, false, true, LONG>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
  (void)hipFuncSetAttribute((const void*)k_row_layer<true, true, true, LONG>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
}
void rowk_setup() {
  rowk_setup_t<false>();
  rowk_setup_t<true>();
}

// whole rows per tile (256 token slots): C <= 256
int rowk_rows_per_tile(int C) { return RT / C; }

int64_t rowk_grid(int64_t ntiles) {
  static int ncu = 0;  // one persistent workgroup per CU
  if (ncu == 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
  }
  return ntiles < ncu ? ntiles : ncu;
}

template <bool LONG>
static void launch_row_layer_t(const RowLayerParams& p, dim3 g, dim3 b, hipStream_t s) {
  if (p.out_qkv) {
    if (p.do_post) hipLaunchKernelGGL((k_row_layer<true, true, true, LONG>), g, b, SMEM_BYTES, s, p);
    else hipLaunchKernelGGL((k_row_layer<true, false, true, LONG>), g, b, SMEM_BYTES, s, p);
  } else if (!p.do_post) {
    hipLaunchKernelGGL((k_row_layer<false, false, true, LONG>), g, b, SMEM_BYTES, s, p);
  } else if (p.do_pre) {
    hipLaunchKernelGGL((k_row_layer<false, true, true, LONG>), g, b, SMEM_BYTES, s, p);
  } else {
    hipLaunchKernelGGL((k_row_layer<false, true, false, LONG>), g, b, SMEM_BYTES, s, p);
  }
}

hipError_t launch_row_layer(const RowLayerParams& p, hipStream_t s, bool inject_fail) {
  const int64_t grid = rowk_grid(p.ntiles);
  if (grid <= 0) return hipSuccess;
  // inject_fail (npfn_debug_fail_row_launch): a block larger than the device allows, so the
  // launch is refused on the host and nothing runs -- the error path's test
  const dim3 g((unsigned)grid), b(inject_fail ? 2048 : 512);
  bool long_rows = false;
  for (int i = 0; i < p.nseg; ++i) long_rows |= p.seg[i].C > 64;
  if (long_rows) launch_row_layer_t<true>(p, g, b, s);
  else launch_row_layer_t<false>(p, g, b, s);
  return hipGetLastError();
}

}  // namespace npfn
