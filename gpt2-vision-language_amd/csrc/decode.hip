// Incremental decoding: single-query attention over a KV cache and a fused
// temperature / top-k / top-p sampler.  Both are latency-bound (one new token per sequence).
//
// attn_decode_kernel: one 256-thread workgroup per (head, sequence) runs attn_decode_body
// (attn_decode.h, which describes the passes) on a strided cache.
// Its IND instance (gvl_attn_decode_beam, beam search) takes the cache row of every key / value
// from an int32 table src[sequence][position]; the plain instance is unchanged by it.
// Its GAP instances (gvl_attn_decode_ragged, prompts of different lengths in one batch) leave
// out the keys of a per-sequence range [gap_lo[sequence], gap_hi): those are never loaded and
// take no part in the max, the sum or the accumulation; the other two instances are unchanged.
// attn_decode_step_kernel (gvl_attn_decode_step, graph-replayed decoding) is the same body again
// with the column of the step read from device memory and the new k / v appended in the launch.
//
// sample_kernel: one 1024-thread workgroup per row; the row (V <= 65536) sits in registers as
// contiguous 64-element chunks.  softmax(logits / T) -> top-k by an 8-bit radix select on the
// probability bits -> top-p by a radix search on probability MASS (the kept set is the
// reference's sorted-cumsum prefix: every token whose preceding cumulative probability is
// <= top_p, gpt2_linear/data.py:117-122) -> inverse-CDF draw of the caller's uniform u in
// token-index order (block prefix scan of the per-thread kept mass).
#include <type_traits>

#include "attn_decode.h"
#include "capi_util.h"
#include "../../include/gvl.h"

namespace {

struct DecP {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  bf16_t* o;
  int64_t Tk, q_sb, k_sb, k_st, v_sb, v_st, o_sb;
  float scale;
  const int32_t* src;  // IND: physical cache row of (sequence, position)
  int64_t src_ld;
};

// GAP: the skipped key range of every sequence, on top of DecP (the instances without GAP take
// DecP itself, so their arguments are what they were).
struct DecGapP : DecP {
  const int32_t* gap_lo;  // per sequence; clamped into [0, gap_hi] by the kernel
  int64_t gap_hi;
};

// The KV policy (attn_decode.h) of a strided cache, for head h of sequence b.
// IND (gvl_attn_decode_beam): the key / value of position t of sequence b come from cache row
// src[b][t], clamped into the cache, instead of row b.
// GAP (gvl_attn_decode_ragged): a key t with glo <= t < ghi is skipped: it is not loaded (a NaN
// or an infinity there cannot reach the output: 0 * NaN is NaN, so a masked score would not do).
// Every other key keeps its thread and every value its thread group and place in the sums, so an
// empty gap gives the bits of the instance without GAP.  A sequence with every key skipped has
// l == 0 and writes zeros.
template <bool IND, bool GAP>
struct CacheKV : BF16Elems<CacheKV<IND, GAP>> {
  static constexpr bool may_be_empty = GAP;
  const bf16_t* kb;  // the head's columns of cache row b (IND: of row 0)
  const bf16_t* vb;
  int64_t k_sb, k_st, v_sb, v_st;
  const int32_t* srow;
  int rmax;
  int64_t glo, ghi;
  GVL_DEV CacheKV(const DecP& p, int h, int b)
      : kb(p.k + (IND ? 0 : b * p.k_sb) + h * 64), vb(p.v + (IND ? 0 : b * p.v_sb) + h * 64),
        k_sb(p.k_sb), k_st(p.k_st), v_sb(p.v_sb), v_st(p.v_st),
        srow(IND ? p.src + b * p.src_ld : nullptr), rmax((int)gridDim.y - 1), glo(0), ghi(0) {}
  GVL_DEV void prologue(int) const {}
  GVL_DEV bool skip(int64_t t) const { return GAP && t >= glo && t < ghi; }
  GVL_DEV int64_t row(int64_t t) const { return IND ? (int64_t)min(max(srow[t], 0), rmax) : 0; }
  GVL_DEV const bf16_t* key(int64_t t) const { return kb + row(t) * k_sb + t * k_st; }
  GVL_DEV const bf16_t* value(int64_t t) const { return vb + row(t) * v_sb + t * v_st; }
};

template <bool IND, bool GAP>
__global__ __launch_bounds__(DEC_NT) void attn_decode_kernel(
    std::conditional_t<GAP, DecGapP, DecP> p) {
  const int h = blockIdx.x, b = blockIdx.y;
  CacheKV<IND, GAP> kv(p, h, b);
  if constexpr (GAP) {
    kv.ghi = p.gap_hi;
    kv.glo = min(max((int64_t)p.gap_lo[b], (int64_t)0), kv.ghi);
  }
  attn_decode_body(p.q + b * p.q_sb + h * 64, p.scale, p.Tk, kv, p.o + b * p.o_sb + h * 64);
}

// gvl_attn_decode_step: the column of this step is read on the device, so a replayed graph can
// launch it with the same arguments every token.
struct StepP {
  const bf16_t* qkv;  // [R, 3C] contiguous: this step's c_attn output
  bf16_t* cache;      // [R, Tmax, 3C], rows 3C apart, sequences cache_sb apart
  bf16_t* o;          // [R, C], rows o_ld apart
  const int32_t* t;   // one int32 on the device: the time-aligned column of this step
  int64_t cache_sb, o_ld, Tmax, C;
  float scale;
  const int32_t* src;  // IND: physical cache row of (sequence, position < *t)
  int64_t src_ld;
  const int32_t* gap_lo;  // GAP
  int64_t gap_hi;
};

// The KV policy (attn_decode.h) of sequence b at column tc: position t < tc is cache row b (IND:
// src[b][t], clamped) as CacheKV presents it, position tc is the sequence's own row of qkv, and
// the workgroup copies its head's k and v of that row into cache[b, tc] before the first barrier
// (AppendKV's append, spec.hip).  skip() is CacheKV's.  Every load of the cache in the launch is
// at a position below tc and every store at tc, so the append races with no load.
template <bool IND, bool GAP>
struct StepKV : BF16Elems<StepKV<IND, GAP>> {
  static constexpr bool may_be_empty = GAP;
  bf16_t* cb;        // cache row b (IND: row 0)
  bf16_t* own;       // cache[b, tc]
  const bf16_t* nw;  // qkv[b]
  int64_t tc, sb, C3, koff, voff;
  const int32_t* srow;
  int rmax;
  int64_t glo, ghi;
  GVL_DEV void prologue(int tid) const {  // append: 8 x 16 B of k, 8 x 16 B of v
    if (tid >= 64 && tid < 80) {
      const int c = tid - 64;
      const int64_t off = (c < 8 ? koff : voff) + (c & 7) * 8;
      *reinterpret_cast<uint4*>(own + off) = *reinterpret_cast<const uint4*>(nw + off);
    }
  }
  GVL_DEV bool skip(int64_t t) const { return GAP && t >= glo && t < ghi; }
  GVL_DEV const bf16_t* row(int64_t t) const {
    if (t >= tc) return nw;
    return cb + (IND ? (int64_t)min(max(srow[t], 0), rmax) * sb : 0) + t * C3;
  }
  GVL_DEV const bf16_t* key(int64_t t) const { return row(t) + koff; }
  GVL_DEV const bf16_t* value(int64_t t) const { return row(t) + voff; }
};

template <bool IND, bool GAP>
__global__ __launch_bounds__(DEC_NT) void attn_decode_step_kernel(StepP p) {
  const int h = blockIdx.x, b = blockIdx.y;
  const int64_t tc = *p.t;
  // (block-uniform) a column outside the cache: neither o nor the cache is written
  if (tc < 0 || tc >= p.Tmax || tc >= DEC_MAXT) return;
  const int64_t C3 = 3 * p.C;
  bf16_t* mine = p.cache + b * p.cache_sb;
  const bf16_t* nw = p.qkv + (int64_t)b * C3;
  StepKV<IND, GAP> kv{{}, IND ? p.cache : mine, mine + tc * C3, nw, tc, p.cache_sb, C3,
                      p.C + h * 64, 2 * p.C + h * 64, IND ? p.src + b * p.src_ld : nullptr,
                      (int)gridDim.y - 1, 0, 0};
  if constexpr (GAP) {
    kv.ghi = p.gap_hi;
    kv.glo = min(max((int64_t)p.gap_lo[b], (int64_t)0), kv.ghi);
  }
  attn_decode_body(nw + h * 64, p.scale, tc + 1, kv, p.o + b * p.o_ld + h * 64);
}

constexpr int SMP_NT = 1024;
constexpr int SMP_E = 64;  // elements per thread: V <= 65536

struct SampP {
  const void* logits;
  int64_t ld, V;
  int f32;
  float inv_temp;
  int top_k;
  float top_p;
  const float* u;
  int64_t* out;
};

// Exclusive prefix sum over the block (SMP_NT threads); `sh` holds SMP_NT/64 floats.
GVL_DEV float block_exscan(float v, float* sh, float* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) sh[w] = x;
  __syncthreads();
  float base = 0.f, tot = 0.f;
#pragma unroll
  for (int i = 0; i < SMP_NT / 64; ++i) {
    if (i < w) base += sh[i];
    tot += sh[i];
  }
  *total = tot;
  return base + x - v;
}

// Keep every element > thr and the first n (in token-index order) of those == thr — the
// reference's sorted order breaks ties by index (a stable sort); zero the rest.  Returns the
// kept mass.  Chunks are contiguous per thread, so a block scan of per-thread tie counts gives
// each tied element its index-order rank.
GVL_DEV float keep_at_least(float (&x)[SMP_E], int E, int64_t i0, int64_t V, float thr,
                            uint32_t n, float* red) {
  float ties = 0.f;
#pragma unroll
  for (int j = 0; j < SMP_E; ++j)
    if (j < E && i0 + j < V && x[j] == thr && x[j] > 0.f) ties += 1.f;
  float tot;
  float rank = block_exscan(ties, red, &tot);
  float z = 0.f;
#pragma unroll
  for (int j = 0; j < SMP_E; ++j) {
    if (x[j] > thr) {
      z += x[j];
    } else if (x[j] == thr && x[j] > 0.f && j < E && i0 + j < V) {
      if (rank < (float)n) z += x[j];
      else x[j] = 0.f;
      rank += 1.f;
    } else {
      x[j] = 0.f;
    }
  }
  return block_sum<SMP_NT>(z, red);
}

__global__ __launch_bounds__(SMP_NT) void sample_kernel(SampP p) {
  __shared__ float red[SMP_NT / 64];
  __shared__ uint32_t hist[256];
  __shared__ float histf[256];
  __shared__ uint32_t sel[2];
  __shared__ int owner;
  __shared__ float c_above;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int E = (int)((p.V + SMP_NT - 1) / SMP_NT);
  const int64_t i0 = (int64_t)tid * E;
  float x[SMP_E];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < SMP_E; ++j) {
    const int64_t i = i0 + j;
    float v = -INFINITY;
    if (j < E && i < p.V) {
      v = p.f32 ? reinterpret_cast<const float*>(p.logits)[row * p.ld + i]
                : bf2f(reinterpret_cast<const bf16_t*>(p.logits)[row * p.ld + i]);
      v *= p.inv_temp;
    }
    x[j] = v;
    mx = fmaxf(mx, v);
  }
  mx = block_max<SMP_NT>(mx, red);
  float z = 0.f;
#pragma unroll
  for (int j = 0; j < SMP_E; ++j) {
    x[j] = (x[j] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((x[j] - mx) * DEC_L2E);
    z += x[j];
  }
  z = block_sum<SMP_NT>(z, red);

  if (p.top_k > 0 && p.top_k < p.V) {  // k-th largest probability: radix select on its bits
    uint32_t prefix = 0, msk = 0;
    uint32_t kk = (uint32_t)p.top_k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < SMP_E; ++j) {
        const uint32_t bits = __float_as_uint(x[j]);
        if (j < E && i0 + j < p.V && (bits & msk) == prefix) atomicAdd(&hist[(bits >> shift) & 255], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t c = 0, chosen = 0;
        for (int bb = 255; bb >= 0; --bb) {
          if (c + hist[bb] >= kk) { chosen = (uint32_t)bb; break; }
          c += hist[bb];
        }
        sel[0] = chosen;
        sel[1] = kk - c;
      }
      __syncthreads();
      prefix |= sel[0] << shift;
      msk |= 255u << shift;
      kk = sel[1];
      __syncthreads();
    }
    z = keep_at_least(x, E, i0, p.V, __uint_as_float(prefix), kk, red);
  }

  if (p.top_p < 1.f) {  // smallest top-mass prefix whose cumulative probability exceeds top_p
    const float target = p.top_p * z;
    uint32_t prefix = 0, msk = 0;
    float above = 0.f;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) histf[tid] = 0.f;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < SMP_E; ++j) {
        const uint32_t bits = __float_as_uint(x[j]);
        if (x[j] > 0.f && (bits & msk) == prefix) atomicAdd(&histf[(bits >> shift) & 255], x[j]);
      }
      __syncthreads();
      if (tid == 0) {
        float c = above;
        uint32_t chosen = 0;
        for (int bb = 255; bb >= 0; --bb) {
          if (c + histf[bb] > target) { chosen = (uint32_t)bb; break; }
          c += histf[bb];
          chosen = (uint32_t)bb;  // (rounding: never crossed -> the lowest bin with mass)
        }
        sel[0] = chosen;
        c_above = c;
      }
      __syncthreads();
      prefix |= sel[0] << shift;
      msk |= 255u << shift;
      above = c_above;
      __syncthreads();
    }
    // above = mass strictly above thr; the sorted list crosses top_p inside the tie group
    // at thr after n = floor((target - above) / thr) + 1 of its (index-ordered) members
    const float thr = __uint_as_float(prefix);
    const float need = thr > 0.f ? floorf((target - above) / thr) + 1.f : 1.f;
    z = keep_at_least(x, E, i0, p.V, thr, (uint32_t)fmaxf(need, 1.f), red);
  }

  // inverse CDF in token-index order
  float s = 0.f;
  int last = 0;
#pragma unroll
  for (int j = 0; j < SMP_E; ++j) {
    s += x[j];
    if (x[j] > 0.f) last = j;
  }
  float tot;
  const float pre = block_exscan(s, red, &tot);
  const float target = p.u[row] * tot;
  if (tid == 0) {
    sel[0] = 0xFFFFFFFFu;  // drawn index
    sel[1] = 0;            // fallback: the highest-index kept token (target rounded to tot)
    owner = -1;
  }
  __syncthreads();
  // The owner of target is the LAST thread with kept mass and pre <= target: the first such
  // thread has pre == 0, so these intervals tile [0, tot) whatever the rounding of the scan.
  // (pre <= target < pre + s per thread does not: fl(pre_i + s_i) != pre_{i+1}, and a target
  // in the gap between them was claimed by nobody and drew the fallback.)
  if (s > 0.f) {
    atomicMax(&sel[1], (uint32_t)(i0 + last));
    if (pre <= target && target < tot) atomicMax(&owner, tid);
  }
  __syncthreads();
  if (tid == owner) {
    float acc = pre;
    int pick = last;  // acc never passes target (rounding): my last kept element
    bool found = false;
#pragma unroll
    for (int j = 0; j < SMP_E; ++j) {
      if (!found && x[j] > 0.f) {
        acc += x[j];
        if (acc > target) {
          pick = j;
          found = true;
        }
      }
    }
    sel[0] = (uint32_t)(i0 + pick);
  }
  __syncthreads();
  if (tid == 0) p.out[row] = (int64_t)(sel[0] != 0xFFFFFFFFu ? sel[0] : sel[1]);
}

}  // namespace

// What the three cache entry points require alike; `fn` names the caller in the message.
static int check_cached(const char* fn, const void* q, const void* k, int64_t k_sb, int64_t k_st,
                        const void* v, int64_t v_sb, int64_t v_st, const void* o, int64_t B,
                        int64_t H, int64_t Tk) {
  GVL_REQUIRE(q && k && v && o, "%s: null buffer", fn);
  GVL_REQUIRE(Tk > 0 && Tk <= DEC_MAXT, "%s: Tk=%lld out of range (1..%d)", fn, (long long)Tk,
              DEC_MAXT);
  GVL_REQUIRE(B >= 0 && B <= 65535 && H >= 0, "%s: B=%lld / H=%lld out of range", fn,
              (long long)B, (long long)H);
  GVL_REQUIRE(k_st % 8 == 0 && v_st % 8 == 0 && k_sb % 8 == 0 && v_sb % 8 == 0 &&
                  gvl::aligned16(k) && gvl::aligned16(v),
              "%s: K/V rows must be 16-byte aligned", fn);
  return 0;
}

template <bool IND, bool GAP>
static int launch_cached(const char* fn, const std::conditional_t<GAP, DecGapP, DecP>& p,
                         int64_t B, int64_t H, gvl_stream_t stream) {
  if (B == 0 || H == 0) return 0;
  hipLaunchKernelGGL((attn_decode_kernel<IND, GAP>), dim3((unsigned)H, (unsigned)B),
                     dim3(DEC_NT), 0, gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK(fn);
  return 0;
}

extern "C" int gvl_attn_decode(const void* q, int64_t q_sb, const void* k, int64_t k_sb,
                               int64_t k_st, const void* v, int64_t v_sb, int64_t v_st, void* o,
                               int64_t o_sb, int64_t B, int64_t H, int64_t Tk, float scale,
                               gvl_stream_t stream) {
  const char* fn = "gvl_attn_decode";
  if (check_cached(fn, q, k, k_sb, k_st, v, v_sb, v_st, o, B, H, Tk)) return -1;
  DecP p{static_cast<const bf16_t*>(q), static_cast<const bf16_t*>(k),
         static_cast<const bf16_t*>(v), static_cast<bf16_t*>(o), Tk, q_sb, k_sb, k_st,
         v_sb, v_st, o_sb, scale, nullptr, 0};
  return launch_cached<false, false>(fn, p, B, H, stream);
}

extern "C" int gvl_attn_decode_beam(const void* q, int64_t q_sb, const void* k, int64_t k_sb,
                                    int64_t k_st, const void* v, int64_t v_sb, int64_t v_st,
                                    void* o, int64_t o_sb, int64_t B, int64_t H, int64_t Tk,
                                    float scale, const int32_t* src, int64_t src_ld,
                                    gvl_stream_t stream) {
  const char* fn = "gvl_attn_decode_beam";
  if (check_cached(fn, q, k, k_sb, k_st, v, v_sb, v_st, o, B, H, Tk)) return -1;
  GVL_REQUIRE(src, "gvl_attn_decode_beam: null src table");
  GVL_REQUIRE(src_ld >= Tk, "gvl_attn_decode_beam: src_ld=%lld < Tk=%lld", (long long)src_ld,
              (long long)Tk);
  DecP p{static_cast<const bf16_t*>(q), static_cast<const bf16_t*>(k),
         static_cast<const bf16_t*>(v), static_cast<bf16_t*>(o), Tk, q_sb, k_sb, k_st,
         v_sb, v_st, o_sb, scale, src, src_ld};
  return launch_cached<true, false>(fn, p, B, H, stream);
}

extern "C" int gvl_attn_decode_ragged(const void* q, int64_t q_sb, const void* k, int64_t k_sb,
                                      int64_t k_st, const void* v, int64_t v_sb, int64_t v_st,
                                      void* o, int64_t o_sb, int64_t B, int64_t H, int64_t Tk,
                                      float scale, const int32_t* src, int64_t src_ld,
                                      const int32_t* gap_lo, int64_t gap_hi,
                                      gvl_stream_t stream) {
  const char* fn = "gvl_attn_decode_ragged";
  if (check_cached(fn, q, k, k_sb, k_st, v, v_sb, v_st, o, B, H, Tk)) return -1;
  GVL_REQUIRE(gap_lo, "gvl_attn_decode_ragged: null gap_lo table");
  GVL_REQUIRE(gap_hi >= 0 && gap_hi <= Tk, "gvl_attn_decode_ragged: gap_hi=%lld outside 0..Tk=%lld",
              (long long)gap_hi, (long long)Tk);
  GVL_REQUIRE(!src || src_ld >= Tk, "gvl_attn_decode_ragged: src_ld=%lld < Tk=%lld",
              (long long)src_ld, (long long)Tk);
  DecGapP p{{static_cast<const bf16_t*>(q), static_cast<const bf16_t*>(k),
             static_cast<const bf16_t*>(v), static_cast<bf16_t*>(o), Tk, q_sb, k_sb, k_st,
             v_sb, v_st, o_sb, scale, src, src ? src_ld : 0},
            gap_lo, gap_hi};
  return src ? launch_cached<true, true>(fn, p, B, H, stream)
             : launch_cached<false, true>(fn, p, B, H, stream);
}

template <bool IND, bool GAP>
static int launch_step(const StepP& p, int64_t R, int64_t H, gvl_stream_t stream) {
  hipLaunchKernelGGL((attn_decode_step_kernel<IND, GAP>), dim3((unsigned)H, (unsigned)R),
                     dim3(DEC_NT), 0, gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK("gvl_attn_decode_step");
  return 0;
}

extern "C" int gvl_attn_decode_step(const void* qkv, void* cache, int64_t cache_sb, int64_t Tmax,
                                    const int32_t* t, void* o, int64_t o_ld, int64_t R, int64_t H,
                                    float scale, const int32_t* src, int64_t src_ld,
                                    const int32_t* gap_lo, int64_t gap_hi, gvl_stream_t stream) {
  GVL_REQUIRE(qkv && cache && o, "gvl_attn_decode_step: null buffer");
  GVL_REQUIRE(t, "gvl_attn_decode_step: null t");
  GVL_REQUIRE(Tmax >= 1 && Tmax <= DEC_MAXT, "gvl_attn_decode_step: Tmax=%lld out of range (1..%d)",
              (long long)Tmax, DEC_MAXT);
  GVL_REQUIRE(R >= 0 && R <= 65535 && H >= 0 && H <= 65535,
              "gvl_attn_decode_step: R=%lld / H=%lld out of range", (long long)R, (long long)H);
  GVL_REQUIRE(cache_sb >= Tmax * 3 * H * 64 && cache_sb % 8 == 0,
              "gvl_attn_decode_step: cache_sb=%lld is no stride of [Tmax, 3C] rows",
              (long long)cache_sb);
  GVL_REQUIRE(o_ld >= H * 64, "gvl_attn_decode_step: o_ld=%lld < C", (long long)o_ld);
  GVL_REQUIRE(gvl::aligned16(qkv) && gvl::aligned16(cache),
              "gvl_attn_decode_step: qkv and cache must be 16-byte aligned");
  GVL_REQUIRE(!src || src_ld >= Tmax, "gvl_attn_decode_step: src_ld=%lld < Tmax=%lld",
              (long long)src_ld, (long long)Tmax);
  GVL_REQUIRE(!gap_lo || (gap_hi >= 0 && gap_hi <= Tmax),
              "gvl_attn_decode_step: gap_hi=%lld outside 0..Tmax=%lld", (long long)gap_hi,
              (long long)Tmax);
  if (R == 0 || H == 0) return 0;
  StepP p{static_cast<const bf16_t*>(qkv), static_cast<bf16_t*>(cache), static_cast<bf16_t*>(o), t,
          cache_sb, o_ld, Tmax, H * 64, scale, src, src ? src_ld : 0, gap_lo, gap_lo ? gap_hi : 0};
  if (gap_lo) return src ? launch_step<true, true>(p, R, H, stream)
                         : launch_step<false, true>(p, R, H, stream);
  return src ? launch_step<true, false>(p, R, H, stream)
             : launch_step<false, false>(p, R, H, stream);
}

extern "C" int gvl_sample(const void* logits, int64_t ld, int32_t logits_fp32, int64_t rows,
                          int64_t V, float temperature, int32_t top_k, float top_p,
                          const float* u, int64_t* out, gvl_stream_t stream) {
  GVL_REQUIRE(logits && u && out, "gvl_sample: null buffer");
  GVL_REQUIRE(V > 0 && V <= (int64_t)SMP_NT * SMP_E, "gvl_sample: V=%lld unsupported", (long long)V);
  GVL_REQUIRE(temperature > 0.f && top_p > 0.f && top_p <= 1.f && top_k >= 0,
              "gvl_sample: bad temperature / top_k / top_p");
  if (rows == 0) return 0;
  SampP p{logits, ld, V, logits_fp32, 1.f / temperature, top_k, top_p, u, out};
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)rows), dim3(SMP_NT), 0, gvl::as_stream(stream),
                     p);
  GVL_LAUNCH_CHECK("gvl_sample");
  return 0;
}
