// Scoring of given token sequences (include/gvl.h gvl_token_logprobs, gvl_sequence_score).
//
// token_logprobs_kernel: one 512-thread block per row, as ce_row_kernel.  The target logit x[t]
// is read up front; one pass over the row in HBM then yields the row maximum and the rank count
// (elements above x[t], plus equal ones at a lower index).  A bf16 row stays in registers (<= 16
// 16-B chunks per thread at V <= 65536, 64 VGPRs), an fp32 row is read a second time, from L2.
// The second pass forms sum exp(x - max) in fp32 (the difference first, then one v_exp_f32, so no
// rounding of a prescaled maximum is shared by every term) and the first index of the maximum.
// HBM-bound: 2*V bytes per bf16 row (derived).  512 threads for the reason ce_row_kernel gives:
// two or more rows resident per CU, one row's reductions under another's loads.
// A row whose address or stride is not 16-B aligned (ld need only be >= V) takes the
// element-by-element loads of the VEC = false instantiation; columns [V, ld) are masked to -inf in
// the registers and never count as logits.
//
// sequence_score_kernel: one 256-thread block per example (group <= 16 sequences); a wave sums one
// sequence at a time, lane l adding positions l, l + 64, ... in order and the 64 partials by a
// fixed xor tree, so the sums do not depend on the launch.  Thread 0 then takes the two argmins.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "capi_util.h"
#include "../../include/gvl.h"

namespace {

constexpr int TL_NT = 512;
constexpr int TL_MAXV = 65536;
constexpr int TL_MAXC = TL_MAXV / 8 / TL_NT;  // 16-B bf16 chunks per thread
constexpr float TL_L2E = 1.4426950408889634f;
constexpr int SS_NT = 256;
constexpr int SS_MAXG = 16;

struct TokP {
  const void* logits;
  int64_t ld, V;
  const int64_t* targets;
  const uint8_t* mask;
  float* logp;
  float* lse;
  int32_t* argmax;
  int32_t* rank;
};

GVL_DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
GVL_DEV int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// The 8 bf16 logits of 16-B chunk c as raw words; columns >= V come back as bf16 -inf (0xFF80)
template <bool VEC>
GVL_DEV uint4 load_bf16_chunk(const bf16_t* row, int c, int64_t V) {
  const int64_t base = (int64_t)c * 8;
  uint32_t w[4];
  if (VEC) {
    const uint4 u = *reinterpret_cast<const uint4*>(row + base);
    if (base + 8 <= V) return u;
    w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (base + 2 * k >= V) w[k] = (w[k] & 0xFFFF0000u) | 0xFF80u;
      if (base + 2 * k + 1 >= V) w[k] = (w[k] & 0x0000FFFFu) | 0xFF800000u;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = base + 2 * k < V ? row[base + 2 * k] : 0xFF80u;
      const uint32_t hi = base + 2 * k + 1 < V ? row[base + 2 * k + 1] : 0xFF80u;
      w[k] = lo | (hi << 16);
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The 4 fp32 logits of 16-B chunk c; columns >= V come back as -inf
template <bool VEC>
GVL_DEV void load_f32_chunk(const float* row, int c, int64_t V, float (&f)[4]) {
  const int64_t base = (int64_t)c * 4;
  if (VEC) {
    const float4 u = *reinterpret_cast<const float4*>(row + base);
    f[0] = u.x; f[1] = u.y; f[2] = u.z; f[3] = u.w;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (base + k >= V) f[k] = -INFINITY;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = base + k < V ? row[base + k] : -INFINITY;
  }
}

// pass 1 over E logits at columns base..: running maximum and the rank count against xt
template <int E>
GVL_DEV void scan_rank(const float (&f)[E], int64_t base, float xt, int64_t tgt, float& mx,
                       int& cnt) {
#pragma unroll
  for (int k = 0; k < E; ++k) {
    mx = fmaxf(mx, f[k]);
    cnt += (f[k] > xt || (f[k] == xt && base + k < tgt)) ? 1 : 0;
  }
}

// pass 2: sum of exp(x - mx), pairwise within the chunk, and the lowest column holding mx
template <int E>
GVL_DEV void scan_sum(const float (&f)[E], int64_t base, float mx, float& s, int& first) {
  float e[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    e[k] = __builtin_amdgcn_exp2f((f[k] - mx) * TL_L2E);
    if (f[k] == mx) first = min(first, (int)(base + k));
  }
#pragma unroll
  for (int w = 1; w < E; w <<= 1)
#pragma unroll
    for (int k = 0; k + w < E; k += 2 * w) e[k] += e[k + w];
  s += e[0];
}

template <bool F32, bool VEC>
__global__ __launch_bounds__(TL_NT) void token_logprobs_kernel(TokP p) {
  constexpr int E = F32 ? 4 : 8;
  constexpr int NW = TL_NT / 64;
  __shared__ float redf[NW];
  __shared__ int redi[2][NW];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t V = p.V;
  const int64_t tgt = p.targets[r];
  // (block-uniform) an ignored or masked row: its logits are not read
  if (tgt == -100 || (p.mask != nullptr && p.mask[r] == 0)) {
    if (tid == 0) {
      if (p.logp) p.logp[r] = 0.f;
      if (p.lse) p.lse[r] = 0.f;
      if (p.argmax) p.argmax[r] = -1;
      if (p.rank) p.rank[r] = -1;
    }
    return;
  }
  const void* row = static_cast<const char*>(p.logits) + r * p.ld * (F32 ? 4 : 2);
  // a target outside [0, V) never indexes the row: NaN compares false everywhere below
  const bool inr = tgt >= 0 && tgt < V;
  float xt = __int_as_float(0x7fc00000);
  if (inr) xt = F32 ? static_cast<const float*>(row)[tgt] : bf2f(static_cast<const bf16_t*>(row)[tgt]);
  const int nch = (int)((V + E - 1) / E);

  float mx = -INFINITY, s = 0.f;
  int cnt = 0, first = INT_MAX;
  if constexpr (F32) {
    const float* frow = static_cast<const float*>(row);
#pragma unroll 4
    for (int c = tid; c < nch; c += TL_NT) {
      float f[E];
      load_f32_chunk<VEC>(frow, c, V, f);
      scan_rank(f, (int64_t)c * E, xt, tgt, mx, cnt);
    }
    mx = block_max<TL_NT, true>(mx, redf);
#pragma unroll 4
    for (int c = tid; c < nch; c += TL_NT) {  // the row again, from L2
      float f[E];
      load_f32_chunk<VEC>(frow, c, V, f);
      scan_sum(f, (int64_t)c * E, mx, s, first);
    }
  } else {
    uint4 buf[TL_MAXC];
#pragma unroll
    for (int i = 0; i < TL_MAXC; ++i) {
      const int c = tid + i * TL_NT;
      if (c < nch) {
        buf[i] = load_bf16_chunk<VEC>(static_cast<const bf16_t*>(row), c, V);
        float f[E];
        unpack8(buf[i], f);
        scan_rank(f, (int64_t)c * E, xt, tgt, mx, cnt);
      }
    }
    mx = block_max<TL_NT, true>(mx, redf);
#pragma unroll
    for (int i = 0; i < TL_MAXC; ++i) {
      const int c = tid + i * TL_NT;
      if (c < nch) {
        float f[E];
        unpack8(buf[i], f);
        scan_sum(f, (int64_t)c * E, mx, s, first);
      }
    }
  }
  s = block_sum<TL_NT, true>(s, redf);
  cnt = wave_sum_i(cnt);
  first = wave_min_i(first);
  if ((tid & 63) == 0) {
    redi[0][tid >> 6] = cnt;
    redi[1][tid >> 6] = first;
  }
  __syncthreads();
  if (tid == 0) {
    int ct = 0, fi = INT_MAX;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      ct += redi[0][i];
      fi = min(fi, redi[1][i]);
    }
    const float lse = mx + logf(s);  // one thread per row: the accurate log costs nothing here
    if (p.logp) p.logp[r] = xt - lse;
    if (p.lse) p.lse[r] = lse;
    if (p.argmax) p.argmax[r] = fi == INT_MAX ? -1 : fi;
    if (p.rank) p.rank[r] = inr ? ct : -1;
  }
}

__global__ __launch_bounds__(SS_NT) void sequence_score_kernel(
    const float* __restrict__ logp, const uint8_t* __restrict__ mask, int64_t T, int group,
    float* __restrict__ sum_nll, int32_t* __restrict__ count, float* __restrict__ mean_nll,
    int32_t* __restrict__ pred_norm, int32_t* __restrict__ pred) {
  __shared__ float ssum[SS_MAXG];
  __shared__ float smean[SS_MAXG];
  __shared__ int scnt[SS_MAXG];
  const int64_t g = blockIdx.x;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int j = w; j < group; j += SS_NT / 64) {  // (wave-uniform)
    const int64_t n = g * group + j;
    const float* lp = logp + n * T;
    const uint8_t* mk = mask ? mask + n * T : nullptr;
    float s = 0.f;
    int c = 0;
    for (int64_t t = l; t < T; t += 64) {
      if (mk == nullptr || mk[t] != 0) {
        s -= lp[t];
        c += 1;
      }
    }
    s = warp_sum(s);
    c = wave_sum_i(c);
    if (l == 0) {
      const float m = s / (float)c;  // 0 / 0 -> nan like torch
      sum_nll[n] = s;
      count[n] = c;
      mean_nll[n] = m;
      ssum[j] = s;
      smean[j] = m;
      scnt[j] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int bn = 0, bs = 0;
    bool empty = scnt[0] == 0;
    for (int j = 1; j < group; ++j) {
      if (smean[j] < smean[bn]) bn = j;
      if (ssum[j] < ssum[bs]) bs = j;
      empty = empty || scnt[j] == 0;
    }
    pred_norm[g] = empty ? -1 : bn;
    pred[g] = empty ? -1 : bs;
  }
}

}  // namespace

extern "C" int gvl_token_logprobs(const void* logits, int64_t ld, int32_t logits_fp32, int64_t rows,
                                  int64_t V, const int64_t* targets, const uint8_t* mask,
                                  float* logp, float* lse, int32_t* argmax, int32_t* rank,
                                  gvl_stream_t stream) {
  GVL_REQUIRE(logits != nullptr, "gvl_token_logprobs: null logits");
  GVL_REQUIRE(targets != nullptr, "gvl_token_logprobs: null targets");
  GVL_REQUIRE(V >= 1 && V <= TL_MAXV, "gvl_token_logprobs: V=%lld out of range (1..%d)",
              (long long)V, TL_MAXV);
  GVL_REQUIRE(ld >= V, "gvl_token_logprobs: ld=%lld < V=%lld", (long long)ld, (long long)V);
  GVL_REQUIRE(rows >= 0 && rows <= 0x7fffffff, "gvl_token_logprobs: rows=%lld out of range",
              (long long)rows);
  if (rows == 0) return 0;
  TokP p{logits, ld, V, targets, mask, logp, lse, argmax, rank};
  const int64_t row_bytes = ld * (logits_fp32 ? 4 : 2);
  const bool vec = gvl::aligned16(logits) && row_bytes % 16 == 0;
  const dim3 grid((unsigned)rows), block(TL_NT);
  hipStream_t s = gvl::as_stream(stream);
  if (logits_fp32) {
    if (vec) hipLaunchKernelGGL((token_logprobs_kernel<true, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((token_logprobs_kernel<true, false>), grid, block, 0, s, p);
  } else {
    if (vec) hipLaunchKernelGGL((token_logprobs_kernel<false, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((token_logprobs_kernel<false, false>), grid, block, 0, s, p);
  }
  GVL_LAUNCH_CHECK("gvl_token_logprobs");
  return 0;
}

extern "C" int gvl_sequence_score(const float* logp, const uint8_t* mask, int64_t N, int64_t T,
                                  int32_t group, float* sum_nll, int32_t* count, float* mean_nll,
                                  int32_t* pred_norm, int32_t* pred, gvl_stream_t stream) {
  GVL_REQUIRE(group >= 1 && group <= SS_MAXG, "gvl_sequence_score: group=%d out of range (1..%d)",
              (int)group, SS_MAXG);
  GVL_REQUIRE(N >= 0 && N % group == 0 && N / group <= 0x7fffffff,
              "gvl_sequence_score: N=%lld must be a multiple of group=%d", (long long)N,
              (int)group);
  GVL_REQUIRE(T >= 0, "gvl_sequence_score: T=%lld is negative", (long long)T);
  GVL_REQUIRE(logp != nullptr || N * T == 0, "gvl_sequence_score: null logp");
  GVL_REQUIRE(sum_nll && count && mean_nll && pred_norm && pred,
              "gvl_sequence_score: null output buffer");
  if (N == 0) return 0;
  hipLaunchKernelGGL(sequence_score_kernel, dim3((unsigned)(N / group)), dim3(SS_NT), 0,
                     gvl::as_stream(stream), logp, mask, T, (int)group, sum_nll, count, mean_nll,
                     pred_norm, pred);
  GVL_LAUNCH_CHECK("gvl_sequence_score");
  return 0;
}
