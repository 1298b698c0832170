// Single-query decode attention: the one workgroup body behind gvl_attn_decode, _beam, _ragged
// (decode.hip), _multi (spec.hip) and _q8 (attn_decode_q8.hip).  Every instance is this text, so
// the bit properties that include/gvl.h states between them hold by construction: a new variant
// is a new KV policy, never a new kernel.
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
// and, since the int8 cache, how its elements come:
//   key_row(t)         the loads of key t, not yet used (the bf16 policies: its row as uint4*)
//   key8(row, c, f)    f[0..8) = elements 8c .. 8c+7 of that key as fp32
//   value_row(t, d8)   the load of elements 8 d8 .. 8 d8+7 of value t, not yet used
//   value8(vrow, f)    those elements as fp32
//   scaled             (static constexpr bool) the elements carry a per-position factor:
//                      score_t = key_scale(row) * sum_d q_d k_td, applied once after the sum
//                      (the factor comes with the key's handle), and the weight of value t is
//                      e_t * value_scale(t), formed once per position in the exponential pass
//   keys_in_flight, values_in_flight   (static constexpr int) how many positions a thread loads
//                      before it uses the first: the sums and their order do not depend on it
//   own_last           (static constexpr bool) the last position (Tk - 1) is the workgroup's own,
//                      served by own_key_row() / own_value_row(d8) and not by the loads of
//                      key_row / value_row; it takes the place in the max, the sum and the
//                      accumulation that its index gives it
// BF16Elems (the three bf16 policies) is the former unpack8 with no factor and one position in
// flight; everything above folds away at compile time and their instances are the instructions
// they were.
#pragma once
#include "common.h"

constexpr int DEC_NT = 256;
constexpr int DEC_MAXT = 4096;  // keys per query: sc[]
constexpr float DEC_L2E = 1.4426950408889634f;

// The element hooks of a policy whose key(t) / value(t) point at 64 bf16.
template <class KV>
struct BF16Elems {
  static constexpr bool scaled = false;
  static constexpr int keys_in_flight = 1, values_in_flight = 1;
  static constexpr bool own_last = false;
  GVL_DEV const uint4* key_row(int64_t t) const {
    return reinterpret_cast<const uint4*>(static_cast<const KV*>(this)->key(t));
  }
  GVL_DEV void key8(const uint4* row, int c, float (&f)[8]) const { unpack8(row[c], f); }
  GVL_DEV const uint4* value_row(int64_t t, int d8) const {
    return reinterpret_cast<const uint4*>(static_cast<const KV*>(this)->value(t) + d8 * 8);
  }
  GVL_DEV void value8(const uint4* v, float (&f)[8]) const { unpack8(*v, f); }
  GVL_DEV float key_scale(const uint4*) const { return 1.f; }
  GVL_DEV float value_scale(int64_t) const { return 1.f; }
};

// qrow: the head's 64 query elements; orow: its 64 outputs; Tk <= DEC_MAXT positions.
template <class KV>
GVL_DEV void attn_decode_body(const bf16_t* qrow, float scale, int64_t Tk, const KV& kv,
                              bf16_t* orow) {
  __shared__ float qs[64];
  __shared__ float sc[DEC_MAXT];
  __shared__ float red[DEC_NT / 64];
  __shared__ float part[32][65];
  constexpr int KF = KV::keys_in_flight, VF = KV::values_in_flight;
  const int tid = threadIdx.x;
  if (tid < 64) qs[tid] = bf2f(qrow[tid]) * (scale * DEC_L2E);
  kv.prologue(tid);
  __syncthreads();
  float q[64];
#pragma unroll
  for (int d = 0; d < 64; ++d) q[d] = qs[d];
  float mx = -INFINITY;
  const int64_t Tl = KV::own_last ? Tk - 1 : Tk;  // the positions that are loaded
  const auto score = [&](const auto& row, int64_t t) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float f[8];
      kv.key8(row, c, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) s = fmaf(q[8 * c + j], f[j], s);
    }
    if constexpr (KV::scaled) s *= kv.key_scale(row);
    sc[t] = s;
    mx = fmaxf(mx, s);
  };
  if constexpr (KF == 1) {  // (kept as its own text: the bf16 instances' instructions)
    for (int64_t t = tid; t < Tl; t += DEC_NT) {
      if (kv.skip(t)) continue;
      const auto row = kv.key_row(t);
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float f[8];
        kv.key8(row, c, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) s = fmaf(q[8 * c + j], f[j], s);
      }
      if constexpr (KV::scaled) s *= kv.key_scale(row);
      sc[t] = s;
      mx = fmaxf(mx, s);
    }
  } else {
    for (int64_t t0 = tid; t0 < Tl; t0 += DEC_NT * KF) {
      decltype(kv.key_row(t0)) row[KF];
      bool on[KF];
#pragma unroll
      for (int u = 0; u < KF; ++u) {  // every load of the sweep before the first use
        const int64_t t = t0 + u * DEC_NT;
        on[u] = (u == 0 || t < Tl) && !kv.skip(t);
        if (on[u]) row[u] = kv.key_row(t);
      }
#pragma unroll
      for (int u = 0; u < KF; ++u)
        if (on[u]) score(row[u], t0 + u * DEC_NT);
    }
  }
  if constexpr (KV::own_last)
    if (tid == (int)(Tl % DEC_NT) && !kv.skip(Tl)) score(kv.own_key_row(), Tl);
  mx = block_max<DEC_NT>(mx, red);
  float l = 0.f;
  if constexpr (!KV::scaled) {
    for (int64_t t = tid; t < Tk; t += DEC_NT) {
      if (kv.skip(t)) continue;
      const float e = __builtin_amdgcn_exp2f(sc[t] - mx);
      sc[t] = e;
      l += e;
    }
  } else {  // sc[t] = the weight of value t; four factors in flight per thread
    for (int64_t t0 = tid; t0 < Tk; t0 += DEC_NT * 4) {
      float vs[4];
      bool on[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t t = t0 + u * DEC_NT;
        on[u] = (u == 0 || t < Tk) && !kv.skip(t);
        if (on[u]) vs[u] = KV::own_last && t == Tl ? kv.own_value_scale() : kv.value_scale(t);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!on[u]) continue;
        const int64_t t = t0 + u * DEC_NT;
        const float e = __builtin_amdgcn_exp2f(sc[t] - mx);
        sc[t] = e * vs[u];
        l += e;
      }
    }
  }
  l = block_sum<DEC_NT>(l, red);  // (its barriers also publish sc[])
  const int d8 = tid & 7, tg = tid >> 3;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const auto weigh = [&](const auto& vrow, int64_t t) {
    float f[8];
    kv.value8(vrow, f);
    const float w = sc[t];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, f[j], acc[j]);
  };
  if constexpr (VF == 1) {
    for (int64_t t = tg; t < Tl; t += 32) {
      if (kv.skip(t)) continue;
      float f[8];
      kv.value8(kv.value_row(t, d8), f);
      const float w = sc[t];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, f[j], acc[j]);
    }
  } else {
    for (int64_t t0 = tg; t0 < Tl; t0 += 32 * VF) {
      decltype(kv.value_row(t0, d8)) vrow[VF];
      bool on[VF];
#pragma unroll
      for (int u = 0; u < VF; ++u) {
        const int64_t t = t0 + u * 32;
        on[u] = (u == 0 || t < Tl) && !kv.skip(t);
        if (on[u]) vrow[u] = kv.value_row(t, d8);
      }
#pragma unroll
      for (int u = 0; u < VF; ++u)
        if (on[u]) weigh(vrow[u], t0 + u * 32);
    }
  }
  // (the group's largest position: after its others, as in the one-at-a-time loop)
  if constexpr (KV::own_last)
    if (tg == (int)(Tl % 32) && !kv.skip(Tl)) weigh(kv.own_value_row(d8), Tl);
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
