// Four-wave deep-ring GEMM for narrow outputs (N = 768 at M = 8064: the caption decoder's
// attn.c_proj / mlp.c_proj forward and c_attn / c_fc / c_proj dX).
//
// Why a fourth kernel: those outputs are 96 tiles of 256x256 (a third of the chip) or 378 of
// 128x128 (1.5 rounds), and the 192x128 tile that fills the chip in one round (42 x 6 = 252
// tiles at M = 8064) ran no faster than 128x128 in the ring kernel (gemm_ring.hip cfg 7): with
// one workgroup of 4 waves per CU there is one wave per SIMD, so every stall is an MFMA bubble,
// and its 4-slot ring keeps only two 32-deep K-steps (~0.35 us of MFMA work) in flight — less
// than an L2/MALL miss.  Here:
//   * tile 192x128, 4 waves of 96x64 (6 x 4 fragments, 24 MFMA 16x16x32 per K-step);
//   * an NS-slot LDS-DMA ring (7 x 20 KiB = 140 KiB): NS - 2 K-steps stay in flight past
//     every barrier (~1 us of MFMA work), one barrier per K-step, counted vmcnt waits;
//   * fragments double-buffered in registers: the 10 ds_reads of step c+1 are issued before
//     the 24 MFMAs of step c, so the LDS latency hides behind them;
//   * persistent over tiles (grid = min(tiles, CUs)) with the ring running across tile
//     boundaries, XCD-contiguous + L2-grouped tile walk, compile-time fused epilogues with
//     16-B stores (gemm_epilogue16, as gemm_pp3_kernel).
// A must be K-contiguous (activations / output gradients); B either layout (nn.Linear weight
// in the forward, the same weight MN-contiguous in dX).  K % 64 == 0.
#include "common.h"
#include "capi_util.h"
#include "gemm_common.h"
#include "gemm_ring.h"
#include "../../include/gvl.h"

namespace {

using namespace gvl_ring;

constexpr int W4_BM = 192, W4_BN = 128;

// Register-staged operand copy of one K-step: this wave's PER 1-KiB pieces (the Step images,
// swizzle on the global source address) loaded to VGPRs, later written lane-linear to LDS.
// (LDS-DMA would need no VGPRs, but each buffer_load...lds costs ~60-185 issue cycles at one
// wave per SIMD, MICROARCH cycle constants: 5 pieces per K-step ~ the whole MFMA budget.)
template <int PER>
GVL_DEV void w4_load(__amdgpu_buffer_rsrc_t rs, const int* off, int kbytes, uint4* v) {
#pragma unroll
  for (int t = 0; t < PER; ++t)
    v[t] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off[t], kbytes, 0));
}
template <int PER, int NWV>
GVL_DEV void w4_store(char* lds, const uint4* v, int wave, int lane) {
#pragma unroll
  for (int t = 0; t < PER; ++t)
    *reinterpret_cast<uint4*>(lds + (t * NWV + wave) * 1024 + lane * 16) = v[t];
}

// 96-row K-contiguous slab of a 32-deep K-step: the B slab of gemm_w4n_kernel (128 x 96 tiles,
// the weight in forward GEMMs) and the A slab of gemm_w4r_kernel.
// 6 KiB of operand in 1-KiB pieces over 4 waves: pieces j = 4t + wave, j < 6 real; waves 2-3's
// second piece (j = 6, 7) is a dummy whose buffer offset is out of range (the load returns
// zeros without touching memory) and whose LDS write lands in a 2 KiB pad no fragment reads,
// so every wave runs the same branch-free staging code.  Image: [96 rows][32] 64-B rows, as
// Step's.  (An MN-contiguous 96-column image for the dX weight was measured slower than the
// 128-column one and is gone: DESIGN, settled variants.)
constexpr uint32_t W4_OOB = 0x7FFFFFF0u;
struct Step96 {
  static constexpr int REAL = 6;
  static constexpr int BYTES = 8 * 1024;  // 6 KiB image + 2 KiB pad for the dummy pieces
  static constexpr int PER = 2;
  static constexpr int NWV = 4;
  GVL_DEV static int64_t elem(int64_t ld, int64_t r0, int64_t k0, int j, int lane) {
    const int row = 16 * j + (lane >> 2);
    return (r0 + row) * ld + k0 + ((lane & 3) ^ f64b(row)) * 8;
  }
  GVL_DEV static void base_offsets(int64_t ld, int64_t r0, int64_t k0, int wave, int lane,
                                   int (&off)[PER]) {
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int j = t * NWV + wave;
      off[t] = j < REAL ? (int)(elem(ld, r0, k0, j, lane) * 2) : (int)W4_OOB;
    }
  }
  GVL_DEV static int step_bytes(int64_t) { return KS * 2; }
  GVL_DEV static short8_t frag(const char* lds, int c0, int lane) {
    const int row = c0 + (lane & 15), ch = lane >> 4;
    return *reinterpret_cast<const short8_t*>(lds + row * 64 + ((ch ^ f64b(row)) << 4));
  }
};
template <int BN, bool MN>
struct W4SlabB {
  using type = Step<BN, MN, 4>;
};
template <>
struct W4SlabB<96, false> {  // (K-contiguous B only: launch_w4)
  using type = Step96;
};
// A slab (K-contiguous): the Step image, or Step96's [96 rows][32] one for 96-row tiles
template <int BM>
struct W4SlabA {
  using type = Step<BM, false, 4>;
};
template <>
struct W4SlabA<96> {
  using type = Step96;
};

// K-steps are 32 deep; the register staging runs P = 3 steps ahead of the LDS writes, the LDS
// ring holds NS = 3 steps (the one being read, the next, the one being written).  Step c:
//   read the fragments of step c+1 (written and published by the previous barrier);
//   write step c+2 from its register set to LDS slot (c+2)%3 (slot of step c-1, whose reads
//   retired before the previous barrier), then reload that set with step c+5;
//   MFMAs of step c; barrier (retires this step's fragment reads and LDS writes).
// The loop body is unrolled 6 times (register set = step % 3, fragment buffer = step % 2, both
// static), so K must be a multiple of 6 steps (K % 192 == 0).
// The scheduler is asked to spread the step's LDS reads, LDS writes and global loads between
// its 24 MFMAs (one wave per SIMD: whatever is not issued in an MFMA's shadow is an MFMA bubble)
// instead of issuing them as one block ahead of the MFMAs: PA+PB rounds of {MFMA, read, MFMA,
// read, MFMA, load, MFMA, write} (at most FM * FN / 4 rounds: the 128 x 96 tile has 12 MFMAs per
// step for 4 loads).  Measured best on the caption shapes of this pattern, no interleave, "reads,
// then writes, then loads, one per MFMA" and "loads first, then reads, then writes".  No
// s_setprio around the MFMAs: it would split the scheduling region.
#define W4_INTERLEAVE()                                                           \
  do {                                                                            \
    _Pragma("unroll") for (int q_ = 0; q_ < (PA + PB < FM * FN / 4 ? PA + PB : FM * FN / 4); ++q_) { \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          \
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                          \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          \
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                          \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          \
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                          \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          \
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                          \
    }                                                                             \
    if constexpr (FM * FN > 4 * (PA + PB))                                        \
      __builtin_amdgcn_sched_group_barrier(0x008, FM * FN - 4 * (PA + PB), 0);    \
  } while (0)

// BM = 192 (6 x 4 fragments per wave) or 128 (4 x 4): the 128-row tile fills the chip when
// 192-row tiles would leave over a quarter of the CUs idle (3968 / 4096-row caption GEMMs).
template <int NS, bool BMN, int EPI, int BM, int BN = W4_BN>
__device__ __forceinline__ void gemm_w4_body(const GemmP& p) {
  constexpr int NW = 4, FM = BM / 32, FN = BN / 32, P = 3;
  static_assert(NS == 3, "ring geometry");
  static_assert(BM == 192 || BM == 128 || (BM == 96 && BN == 128), "tile rows");
  static_assert(BN == 128 || (BN == 96 && BM == 128), "tile columns");
  using SA = typename W4SlabA<BM>::type;
  using SB = typename W4SlabB<BN, BMN>::type;
  constexpr int SLOT = SA::BYTES + SB::BYTES;
  constexpr int PA = SA::PER, PB = SB::PER;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int arow = (wave >> 1) * (BM / 2), bcol = (wave & 1) * (BN / 2);

  const int total = p.tiles_m * p.tiles_n;
  const int G = gridDim.x, b = blockIdx.x;
  const int ntl = (total - b + G - 1) / G;
  const int nks = (int)(p.K / KS);
  auto tile_coords = [&](int t, int64_t& m0, int64_t& n0) {
    const int vid = b + t * G;
    const int q8 = total >> 3, r8 = total & 7, xcd = vid & 7;
    const int work = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (vid >> 3);
    int sp, tm, tn;
    gemm_tile_of(work, 1, p.tiles_m, p.tiles_n, p.group, sp, tm, tn);
    m0 = (int64_t)tm * BM;
    n0 = (int64_t)tn * BN;
  };

  const int64_t b_rows = BMN ? p.K : p.N;
  const __amdgpu_buffer_rsrc_t ra = uniform_rsrc(p.A, p.M * p.lda * 2);
  const __amdgpu_buffer_rsrc_t rb = uniform_rsrc(p.B, b_rows * p.ldb * 2);
  const int sa_step = SA::step_bytes(p.lda), sb_step = SB::step_bytes(p.ldb);
  int is_t = 0, is_k = 0;  // load cursor (steps are loaded strictly in order)
  int offa[PA], offb[PB];
  {
    int64_t m0, n0;
    tile_coords(0, m0, n0);
    SA::base_offsets(p.lda, m0, 0, wave, lane, offa);
    SB::base_offsets(p.ldb, n0, 0, wave, lane, offb);
  }
  uint4 st[P][PA + PB];
// Loads and LDS writes past the last step are issued anyway (they re-read the last tile's
// first steps into a slot nobody reads again): a branch around them would make hipcc's
// vmcnt bookkeeping assume the newest loads belong to the set being written and wait for
// all of them (no loads left in flight).
#define GVL_W4_LOAD(SET)                                                        \
  do {                                                                          \
    w4_load<PA>(ra, offa, is_k * sa_step, st[SET]);                             \
    w4_load<PB>(rb, offb, is_k * sb_step, st[SET] + PA);                        \
    if (++is_k == nks) {                                                        \
      is_k = 0;                                                                 \
      if (++is_t < ntl) {                                                       \
        int64_t m0_, n0_;                                                       \
        tile_coords(is_t, m0_, n0_);                                            \
        SA::base_offsets(p.lda, m0_, 0, wave, lane, offa);                      \
        SB::base_offsets(p.ldb, n0_, 0, wave, lane, offb);                      \
      }                                                                         \
    }                                                                           \
  } while (0)
#define GVL_W4_WRITE(C, SET)  /* step C lives in LDS slot C % 3 == SET */     \
  do {                                                                          \
    char* slot_ = smem + (SET) * SLOT;                                          \
    w4_store<PA, NW>(slot_, st[SET], wave, lane);                               \
    w4_store<PB, NW>(slot_ + SA::BYTES, st[SET] + PA, wave, lane);              \
  } while (0)

  float4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

  float alpha = p.alpha;
  if (p.alpha_ptr) alpha *= *p.alpha_ptr;
  int64_t cu_m0, cu_n0;
  tile_coords(0, cu_m0, cu_n0);
  EpiPre<FM, FN, EPI> pre;
  pre.load_bias(p, cu_n0 + bcol, lane);

  // prologue: steps 0..2 into sets 0..2; steps 0, 1 written; sets 0, 1 reloaded with 3, 4
  GVL_W4_LOAD(0);
  GVL_W4_LOAD(1);
  GVL_W4_LOAD(2);
  GVL_W4_WRITE(0, 0);
  GVL_W4_LOAD(0);
  GVL_W4_WRITE(1, 1);
  GVL_W4_LOAD(1);
  barrier_lds();
  short8_t af[FM], bf[FN], an[FM], bn[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) bf[j] = SB::frag(smem + SA::BYTES, bcol + 16 * j, lane);
#pragma unroll
  for (int i = 0; i < FM; ++i) af[i] = SA::frag(smem, arow + 16 * i, lane);

#define GVL_W4_STEP(C, SET, CA, CB, NA, NB)                                                 \
  do {                                                                                      \
    { /* step C+1 in slot (SET + 2) % 3 */                                                  \
      const char* sl_ = smem + (((SET) + 2) % 3) * SLOT;                                    \
      _Pragma("unroll") for (int j = 0; j < FN; ++j)                                        \
          NB[j] = SB::frag(sl_ + SA::BYTES, bcol + 16 * j, lane);                           \
      _Pragma("unroll") for (int i = 0; i < FM; ++i) NA[i] = SA::frag(sl_, arow + 16 * i, lane); \
    }                                                                                       \
    GVL_W4_WRITE((C) + 2, SET);                                                             \
    GVL_W4_LOAD(SET);                                                                       \
    _Pragma("unroll") for (int i = 0; i < FM; ++i)                                          \
        _Pragma("unroll") for (int j = 0; j < FN; ++j)                                      \
            acc[i][j] = mfma16(CB[j], CA[i], acc[i][j]);                                    \
    W4_INTERLEAVE();                                                                        \
    barrier_lds();                                                                          \
  } while (0)

  int c = 0;
  for (int t = 0; t < ntl; ++t) {
    for (int k = 0; k < nks; k += 6, c += 6) {
      GVL_W4_STEP(c, 2, af, bf, an, bn);
      GVL_W4_STEP(c + 1, 0, an, bn, af, bf);
      GVL_W4_STEP(c + 2, 1, af, bf, an, bn);
      GVL_W4_STEP(c + 3, 2, an, bn, af, bf);
      GVL_W4_STEP(c + 4, 0, af, bf, an, bn);
      GVL_W4_STEP(c + 5, 1, an, bn, af, bf);
    }
    gemm_epilogue16<FM, FN, EPI>(p, acc, cu_m0 + arow, cu_n0 + bcol, lane, alpha, pre);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    if (t + 1 < ntl) {
      tile_coords(t + 1, cu_m0, cu_n0);
      pre.load_bias(p, cu_n0 + bcol, lane);
    }
  }
#undef GVL_W4_STEP
#undef GVL_W4_WRITE
#undef GVL_W4_LOAD
}

// Two kernel names (rocprofv3 / the bench timer tell them apart): 192-row and 128-row tiles.
template <int NS, bool BMN, int EPI>
__global__ __launch_bounds__(256, 1) void gemm_w4_kernel(GemmP p) {
  gemm_w4_body<NS, BMN, EPI, 192>(p);
}
template <int NS, bool BMN, int EPI>
__global__ __launch_bounds__(256, 1) void gemm_w4m_kernel(GemmP p) {
  gemm_w4_body<NS, BMN, EPI, 128>(p);
}
template <int NS, bool BMN, int EPI>
__global__ __launch_bounds__(256, 1) void gemm_w4n_kernel(GemmP p) {
  gemm_w4_body<NS, BMN, EPI, 128, 96>(p);
}
template <int NS, bool BMN, int EPI>
__global__ __launch_bounds__(256, 1) void gemm_w4r_kernel(GemmP p) {
  gemm_w4_body<NS, BMN, EPI, 96, 128>(p);
}

constexpr int W4_NS = 3;  // LDS ring slots (gemm_w4_body's ring geometry)

// the kernel of a tile shape (if constexpr: only the chosen one is instantiated)
template <int BM, int BN, bool BMN, int EPI>
constexpr auto w4_kernel_of() {
  if constexpr (BN == 96) return gemm_w4n_kernel<W4_NS, BMN, EPI>;
  else if constexpr (BM == 96) return gemm_w4r_kernel<W4_NS, BMN, EPI>;
  else if constexpr (BM == 192) return gemm_w4_kernel<W4_NS, BMN, EPI>;
  else return gemm_w4m_kernel<W4_NS, BMN, EPI>;
}
template <int BM, int BN>
constexpr const char* w4_kernel_name() {
  return BN == 96 ? "gemm_w4n_kernel" : BM == 96 ? "gemm_w4r_kernel" : BM == 192 ? "gemm_w4_kernel" : "gemm_w4m_kernel";
}

template <bool BMN, int EPI, int BM, int BN = W4_BN>
int launch_w4_bm(const GemmP& p0, const gvl::GemmSink& k) {
  constexpr int NS = W4_NS;
  if (gvl::gemm_name_only(k, "%s<%d, %s, %d>", w4_kernel_name<BM, BN>(), NS, gvl::tf(BMN), EPI)) return 0;
  GemmP p = p0;
  p.tiles_m = (int)((p.M + BM - 1) / BM);
  p.tiles_n = (int)((p.N + BN - 1) / BN);
  p.splits = 1;
  p.kper = p.K;
  constexpr int slot = W4SlabA<BM>::type::BYTES + W4SlabB<BN, BMN>::type::BYTES;
  constexpr int lds = NS * slot;
  auto kern = w4_kernel_of<BM, BN, BMN, EPI>();
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr_set = true;
  }
  const int total = p.tiles_m * p.tiles_n;
  const int grid = total < gvl::num_cus() ? total : gvl::num_cus();
  gvl::launch_timed(kern, dim3(grid), dim3(256), lds, k.stream, p);
  return 0;
}

// 128-row tiles where 192-row ones fill under 3/4 of the CUs and 128-row ones fill more
bool w4_use128(const GemmP& p) {
  const int64_t cus = gvl::num_cus(), tn = (p.N + W4_BN - 1) / W4_BN;
  const int64_t t192 = (p.M + 191) / 192 * tn, t128 = (p.M + 127) / 128 * tn;
  return t192 * 4 < cus * 3 && t128 > t192 && t128 <= cus;
}

// 128 x 96 tiles (gemm_w4n_kernel) where 128-row tiles are used and 96-column ones fill more
// of the chip in one round: the cross-att decoder's 3968 text rows (186 -> 248 tiles at
// N = 768) and the Q-Former bridge's 4096 query rows (192 -> 256).  A CU streams 224 operand
// rows per K-step instead of 256 for its (smaller) tile, so a one-round launch of these shapes,
// paced by the per-CU operand stream, ends ~1/8 sooner.  Measured
// (profiles/r6/w4n_bn96_r6c.txt, 3968 / 4096 rows): the forward products (K-contiguous weight)
// gain 8-10 % (attn.c_proj + bias + residual 16.3 -> 14.5 us, mlp.c_proj 39.1 -> 35.3), the dX
// ones (MN-contiguous weight, whose 32-column image is fetched as 64-B row segments) lose 6-8 %
// (c_fc.dX 35.8 -> 38.5), so only K-contiguous B takes them (launch_w4).
bool w4_use96(const GemmP& p) {
  if (!w4_use128(p)) return false;
  const int64_t cus = gvl::num_cus(), tm = (p.M + 127) / 128;
  const int64_t t128 = tm * ((p.N + 127) / 128), t96 = tm * ((p.N + 95) / 96);
  return t96 > t128 && t96 <= cus;
}

// 96 x 128 tiles (gemm_w4r_kernel) for the dX products (MN-contiguous weight, plain epilogue)
// where 128-row tiles are used and 96-row ones fill more of the chip in one round: the cross-att
// decoder's 3968 text rows, 186 -> 252 tiles at N = 768.  The 128-column B image keeps its full
// 256-B rows (the 96-column one of gemm_w4n_kernel lost on dX: 64-B row segments); the A slab is
// Step96's [96][32] image (two dummy pieces).
bool w4_use96r(const GemmP& p) {
  if (!w4_use128(p)) return false;
  const int64_t cus = gvl::num_cus(), tn = (p.N + 127) / 128;
  const int64_t t128 = (p.M + 127) / 128 * tn, t96 = (p.M + 95) / 96 * tn;
  return t96 > t128 && t96 <= cus;
}

template <bool BMN, int EPI>
int launch_w4(const GemmP& p, const gvl::GemmSink& s) {
  if constexpr (BMN && EPI == EPI_PLAIN) {
    if (w4_use96r(p)) return launch_w4_bm<BMN, EPI, 96, 128>(p, s);
  }
  if constexpr (!BMN) {
    if (w4_use96(p)) return launch_w4_bm<BMN, EPI, 128, 96>(p, s);
  }
  return w4_use128(p) ? launch_w4_bm<BMN, EPI, 128>(p, s) : launch_w4_bm<BMN, EPI, 192>(p, s);
}

// The four-wave kernels' epilogue kind: gemm_epi_kind, plus the gated residual (EPI_GATE_RES:
// bias, residual, gate and the un-gated branch stored to pre_out; no dropout / activation) that
// every other family runs on the generic epilogue.  Before round 5 the cross-att decoder's 12
// gated xattn.c_proj GEMMs per step (3968 x 768 x 768) fell to the 128 x 128 ring kernel's
// runtime-flag epilogue for that reason: 32 us each, 0.058 of peak.
int w4_epi_kind(const GemmP& p) {
  if (p.gate && p.bias && p.residual && p.pre_out && !p.has_drop && !p.c_f32 && !p.act &&
      !p.dact)
    return EPI_GATE_RES;
  return gvl::gemm_epi_kind(p);
}

template <bool BMN>
int launch_w4_epi(const GemmP& p, const gvl::GemmSink& s) {
  switch (w4_epi_kind(p)) {
    case EPI_PLAIN: return launch_w4<BMN, EPI_PLAIN>(p, s);
    case EPI_BIAS: return launch_w4<BMN, EPI_BIAS>(p, s);
    case EPI_BIAS_RES: return launch_w4<BMN, EPI_BIAS_RES>(p, s);
    case EPI_BIAS_ACT: return launch_w4<BMN, EPI_BIAS_ACT>(p, s);
    case EPI_DACT: return launch_w4<BMN, EPI_DACT>(p, s);
    case EPI_RES: return launch_w4<BMN, EPI_RES>(p, s);
    case EPI_BIAS_ACT_ERF: return launch_w4<BMN, EPI_BIAS_ACT_ERF>(p, s);
    case EPI_DACT_ERF: return launch_w4<BMN, EPI_DACT_ERF>(p, s);
    case EPI_BIAS_ACT_D: return launch_w4<BMN, EPI_BIAS_ACT_D>(p, s);
    case EPI_BIAS_ACT_ERF_D: return launch_w4<BMN, EPI_BIAS_ACT_ERF_D>(p, s);
    case EPI_MUL: return launch_w4<BMN, EPI_MUL>(p, s);
    case EPI_BIAS_DROP_RES: return launch_w4<BMN, EPI_BIAS_DROP_RES>(p, s);
    case EPI_GATE_RES: return launch_w4<BMN, EPI_GATE_RES>(p, s);
    default: return -1;
  }
}

}  // namespace

namespace gvl {

// Shapes it takes by default: narrow outputs (N <= 1024) whose 256x256 tiling leaves most CUs
// idle and whose 192x128 tiling fills at least half the chip.
bool gemm_w4_plan(const GemmP& p, int a_mn, bool force) {
  if (a_mn || p.c_f32 || p.K % (6 * KS) != 0 || p.N % 8 != 0 || p.ldc % 8 != 0) return false;
  if (p.pre_out && (p.ldp % 8 != 0 || (reinterpret_cast<uintptr_t>(p.pre_out) & 15))) return false;
  if (w4_epi_kind(p) == EPI_GEN || w4_epi_kind(p) == EPI_BIAS_QGELU) return false;
  if (force) return true;
  // (not the short-K wide outputs, K <= 1024, N <= 4096: c_attn / c_fc forward, mlp.c_proj dX,
  // whose 192x256 ping-pong tiles run only 24 K-steps each — measured slower here,
  // profiles/r2/r2i/w4s_shapes.txt: 575 vs 790 TF/s at M = 16384)
  const int64_t cus = num_cus();
  const int64_t t256 = ((p.M + 255) / 256) * ((p.N + 255) / 256);
  const int64_t tw4 = ((p.M + W4_BM - 1) / W4_BM) * ((p.N + W4_BN - 1) / W4_BN);
  if (p.N > 1024 || t256 >= 160 || tw4 > cus) return false;
  if (tw4 * 4 >= cus * 3) return true;
  // 40-75 % of the CUs (the cross-att decoder's 3968 text rows: 126 tiles) only with a K short
  // enough that one tile per CU beats splitting K (the caption lm_head dX, K = 50304, and the
  // cross-att batched kv_proj dX, K = 18432, do not)
  return tw4 * 5 >= cus * 2 && p.K <= 4096;
}

int gemm_w4_launch(const GemmP& p, int b_mn, const GemmSink& s) {
  if (!w4_use128(p) && gemm_w4d_ok(p)) {
    // direct-A tiles walk all column tiles of a row block before the next one, so an XCD reads
    // each A row block once: HBM bytes per Q-Former dX launch 104 -> 80 MB at equal time
    // (profiles/r3/w4d_group_ab_r3s2.txt)
    GemmP q = p;
    q.group = 1;
    return gemm_w4d_launch(q, b_mn, s);
  }
  return b_mn ? launch_w4_epi<true>(p, s) : launch_w4_epi<false>(p, s);
}

}  // namespace gvl
