// Single-query decode attention: the one workgroup body behind gvl_attn_decode, _beam, _ragged
// (decode.hip) and _multi (spec.hip).  Every instance is this text, so the bit properties that
// include/gvl.h states between them hold by construction: a new variant is a new KV policy,
// never a new kernel.
//
// One 256-thread workgroup per query.  Pass 1 scores every key against the query (one key per
// thread, 8 x 16-B loads of its 64-dim row) into an LDS score array, block max/sum in fp32;
// pass 2 accumulates p_t * v_t with 8 threads per value row (16-B loads, 32 rows in flight per
// sweep) and folds the 32 partial rows in LDS.
//
// A KV policy says where the keys and values are:
//   key(t), value(t)   the 64 bf16 of this head's key / value at position t (16-byte aligned)
//   skip(t)            position t is left out: never loaded, no part in max, sum or accumulation
//   may_be_empty       (static constexpr bool) skip() may leave no key at all: then l == 0 and
//                      the output is zeros; without it the division is unguarded
//   prologue(tid)      runs before the first barrier (multi's fused append; else empty)
#pragma once
#include "common.h"

constexpr int DEC_NT = 256;
constexpr int DEC_MAXT = 4096;  // keys per query: sc[]
constexpr float DEC_L2E = 1.4426950408889634f;

// qrow: the head's 64 query elements; orow: its 64 outputs; Tk <= DEC_MAXT positions.
template <class KV>
GVL_DEV void attn_decode_body(const bf16_t* qrow, float scale, int64_t Tk, const KV& kv,
                              bf16_t* orow) {
  __shared__ float qs[64];
  __shared__ float sc[DEC_MAXT];
  __shared__ float red[DEC_NT / 64];
  __shared__ float part[32][65];
  const int tid = threadIdx.x;
  if (tid < 64) qs[tid] = bf2f(qrow[tid]) * (scale * DEC_L2E);
  kv.prologue(tid);
  __syncthreads();
  float q[64];
#pragma unroll
  for (int d = 0; d < 64; ++d) q[d] = qs[d];
  float mx = -INFINITY;
  for (int64_t t = tid; t < Tk; t += DEC_NT) {
    if (kv.skip(t)) continue;
    const uint4* row = reinterpret_cast<const uint4*>(kv.key(t));
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float f[8];
      unpack8(row[c], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) s = fmaf(q[8 * c + j], f[j], s);
    }
    sc[t] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_max<DEC_NT>(mx, red);
  float l = 0.f;
  for (int64_t t = tid; t < Tk; t += DEC_NT) {
    if (kv.skip(t)) continue;
    const float e = __builtin_amdgcn_exp2f(sc[t] - mx);
    sc[t] = e;
    l += e;
  }
  l = block_sum<DEC_NT>(l, red);  // (its barriers also publish sc[])
  const int d8 = tid & 7, tg = tid >> 3;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t t = tg; t < Tk; t += 32) {
    if (kv.skip(t)) continue;
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(kv.value(t) + d8 * 8), f);
    const float w = sc[t];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, f[j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[tg][d8 * 8 + j] = acc[j];
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 32; ++g) s += part[g][tid];
    if constexpr (KV::may_be_empty) s = l > 0.f ? s / l : 0.f;
    else s = s / l;
    orow[tid] = f2bf(s);
  }
}
