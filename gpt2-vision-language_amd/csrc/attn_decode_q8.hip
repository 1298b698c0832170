// Int8 KV cache for decoding (include/gvl.h gvl_kv_quantize_i8, gvl_attn_decode_q8): the keys
// and values of a step are quantised as they are appended and dequantised inside the attention.
//
// Format: gvl_quantize_rows_i8's, one "row" being one head's 64-wide key or value vector at one
// position.  Per layer kv8 int8 [rows, Tmax, 2C] (k heads, then v heads) and kvs fp32
// [rows, Tmax, 2H] (k scales, then v scales).  The k and v thirds of a c_attn row are 2H
// consecutive 64-wide vectors, vector j going to kv8 columns 64 j .. and kvs column j.
//
// quant64: one wave quantises one vector, lane = element.  Both the bulk quantiser (the
// prefill) and the fused append of a step run it, so they write the same bytes.
//
// attn_decode_q8_kernel: attn_decode_body (attn_decode.h) with the Q8KV policy.  The workgroup
// of (head h, sequence b) quantises that head's new k (wave 1) and v (wave 2) of qkv[b], stores
// them to column tc of the cache and stages them in LDS; position tc is then served from LDS
// (own_last), so the step attends its own position in quantised form without reading back a
// store of the same launch.  Every load of the cache is at a position below tc and every store
// at tc.  DESIGN 3y has the layout, the assembly checks and the measurements.
#include <type_traits>

#include "attn_decode.h"
#include "capi_util.h"
#include "../../include/gvl.h"

namespace {

// One 64-wide bf16 vector per wave, x the element of this lane (raw bf16 bits).  Returns the
// lane's quantised element and, in *scale, the vector's scale (the same in every lane).
// absmax over the bf16 magnitudes compared as integers (a NaN or an infinity wins and reaches
// the scale), scale = absmax / 127 and q = clamp(rint(x / scale), -127, 127), both divisions
// correctly rounded; a zero vector has scale 0 and q 0 (quantize_rows_i8_kernel, linear_w8.hip).
GVL_DEV int8_t quant64(bf16_t x, float* scale) {
  uint32_t mx = x & 0x7fffu;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, 64);
    mx = mx > other ? mx : other;
  }
  const float s = __fdiv_rn(bf2f(mx), 127.f);
  *scale = s;
  float r = 0.f;
  if (mx != 0u) r = fminf(fmaxf(rintf(__fdiv_rn(bf2f(x), s)), -127.f), 127.f);
  return (int8_t)(int)r;
}

constexpr int KVQ_NT = 256;

struct KvqP {
  const bf16_t* qkv;
  int8_t* kv8;
  float* kvs;
  int64_t qkv_sb, qkv_st, kv8_sb, kvs_sb, S, H, col0, total;
};

// One wave per (sequence b, position s, vector j of the 2H): no LDS, no barrier.
__global__ __launch_bounds__(KVQ_NT) void kv_quantize_i8_kernel(KvqP p) {
  const int lane = threadIdx.x & 63;
  const int64_t vec = (int64_t)blockIdx.x * (KVQ_NT / 64) + (threadIdx.x >> 6);
  if (vec >= p.total) return;  // (wave-uniform)
  const int64_t H2 = 2 * p.H;
  const int64_t j = vec % H2, bs = vec / H2;
  const int64_t s = bs % p.S, b = bs / p.S;
  const bf16_t x = p.qkv[b * p.qkv_sb + s * p.qkv_st + (p.H + j) * 64 + lane];
  float sc;
  const int8_t q = quant64(x, &sc);
  const int64_t col = p.col0 + s;
  p.kv8[b * p.kv8_sb + (col * H2 + j) * 64 + lane] = q;
  if (lane == 0) p.kvs[b * p.kvs_sb + col * H2 + j] = sc;
}

struct Q8P {
  const bf16_t* qkv;  // [R, 3C] contiguous: this step's c_attn output
  int8_t* kv8;        // [R, Tmax, 2C], rows 2C apart, sequences kv8_sb apart
  float* kvs;         // [R, Tmax, 2H], rows 2H apart, sequences kvs_sb apart
  bf16_t* o;          // [R, C], rows o_ld apart
  const int32_t* t_dev;  // the column of this step on the device, or null: then t
  int64_t t, kv8_sb, kvs_sb, o_ld, Tmax, H;
  float scale;
  const int32_t* src;  // IND: physical cache row of (sequence, position < tc)
  int64_t src_ld;
  const int32_t* gap_lo;  // GAP
  int64_t gap_hi;
};

// What the workgroup stages of its own position: the quantised k and v and their scales.
struct Q8Own {
  uint32_t k[16];
  uint32_t v[16];
  float ks, vs;
};
// (typed as LDS, so that its reads can never be folded with a cache load into a flat load)
typedef __attribute__((address_space(3))) const Q8Own lds_q8own_t;

// sign-extended byte j of w as fp32 (one v_cvt_f32_i32 with an sdwa byte select)
GVL_DEV float i8f(uint32_t w, int j) { return (float)(int8_t)(w >> (8 * j)); }

// The KV policy (attn_decode.h) of sequence b, head h at column tc over an int8 cache: position
// t < tc is row b of kv8 / kvs (IND: row src[b][t], clamped), position tc the workgroup's own
// staged vectors.  skip() is CacheKV's (decode.hip): a skipped position is never loaded, neither
// its bytes nor its scales, so a NaN scale there cannot reach the output.
template <bool IND, bool GAP>
struct Q8KV {
  static constexpr bool may_be_empty = GAP;
  static constexpr bool scaled = true;
  // A thread has 8 bytes per value row to load where the bf16 policies have 16: eight rows in
  // flight per thread (the key pass, with the query in 64 VGPRs, has no registers for more
  // than one key: DESIGN 3y).
  static constexpr int keys_in_flight = 1, values_in_flight = 8;
  static constexpr bool own_last = true;
  struct KeyRow {
    uint4 w[4];
    float ks;  // the position's key scale
  };
  const int8_t* kb;  // the head's k columns of cache row b (IND: row 0); v is C further
  const float* sb;   // the head's k scale of cache row b (IND: row 0); v is H further
  lds_q8own_t* own;  // the staged own position
  int64_t tc, kv8_sb, kvs_sb, C, H;
  const int32_t* srow;
  int rmax;
  int64_t glo, ghi;
  // the append, fused: wave 1 the key, wave 2 the value (wave 0 stages the query)
  const bf16_t* nw;  // the head's q of qkv[b]; k is C further, v 2C
  int8_t* own8;      // the head's k columns of kv8[b, tc]
  float* owns;       // the head's k scale of kvs[b, tc]
  Q8Own* stage;
  GVL_DEV void prologue(int tid) const {
    const int w = tid >> 6, lane = tid & 63;
    if (w != 1 && w != 2) return;  // (wave-uniform)
    const bool isv = w == 2;
    float s;
    const int8_t q = quant64(nw[(isv ? 2 * C : C) + lane], &s);
    own8[(isv ? C : 0) + lane] = q;
    reinterpret_cast<int8_t*>(isv ? stage->v : stage->k)[lane] = q;
    if (lane == 0) {
      owns[isv ? H : 0] = s;
      (isv ? stage->vs : stage->ks) = s;
    }
  }
  GVL_DEV bool skip(int64_t t) const { return GAP && t >= glo && t < ghi; }
  GVL_DEV int64_t row(int64_t t) const { return IND ? (int64_t)min(max(srow[t], 0), rmax) : 0; }
  GVL_DEV KeyRow key_row(int64_t t) const {  // t < tc; 64 int8: 4 x 16 B
    KeyRow r;
    const int64_t rw = row(t);
    const uint4* g = reinterpret_cast<const uint4*>(kb + rw * kv8_sb + t * 2 * C);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = g[i];
    r.ks = sb[rw * kvs_sb + t * 2 * H];
    return r;
  }
  GVL_DEV KeyRow own_key_row() const {  // position tc, from LDS
    KeyRow r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      r.w[i] = make_uint4(own->k[4 * i], own->k[4 * i + 1], own->k[4 * i + 2], own->k[4 * i + 3]);
    r.ks = own->ks;
    return r;
  }
  GVL_DEV void key8(const KeyRow& r, int c, float (&f)[8]) const {
    const uint4& u = r.w[c >> 1];
    const uint32_t lo = (c & 1) ? u.z : u.x, hi = (c & 1) ? u.w : u.y;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[j] = i8f(lo, j);
      f[4 + j] = i8f(hi, j);
    }
  }
  // 8 threads per value row, 8 B each: the thread groups and the fold of the bf16 policies
  GVL_DEV uint2 value_row(int64_t t, int d8) const {  // t < tc
    return *reinterpret_cast<const uint2*>(kb + row(t) * kv8_sb + t * 2 * C + C + d8 * 8);
  }
  GVL_DEV uint2 own_value_row(int d8) const {
    return make_uint2(own->v[2 * d8], own->v[2 * d8 + 1]);
  }
  GVL_DEV void value8(const uint2& u, float (&f)[8]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[j] = i8f(u.x, j);
      f[4 + j] = i8f(u.y, j);
    }
  }
  GVL_DEV float key_scale(const KeyRow& r) const { return r.ks; }
  GVL_DEV float value_scale(int64_t t) const { return sb[row(t) * kvs_sb + t * 2 * H + H]; }
  GVL_DEV float own_value_scale() const { return own->vs; }
};

template <bool IND, bool GAP>
__global__ __launch_bounds__(DEC_NT) void attn_decode_q8_kernel(Q8P p) {
  __shared__ Q8Own own;
  const int h = blockIdx.x, b = blockIdx.y;
  const int64_t tc = p.t_dev ? (int64_t)*p.t_dev : p.t;
  // (block-uniform) a column outside the cache: neither o nor the cache is written
  if (tc < 0 || tc >= p.Tmax || tc >= DEC_MAXT) return;
  const int64_t C = p.H * 64;
  const bf16_t* nw = p.qkv + (int64_t)b * 3 * C + h * 64;
  int8_t* mine8 = p.kv8 + b * p.kv8_sb + h * 64;
  float* mines = p.kvs + b * p.kvs_sb + h;
  Q8KV<IND, GAP> kv{IND ? p.kv8 + h * 64 : mine8,
                    IND ? p.kvs + h : mines,
                    (lds_q8own_t*)&own,
                    tc,
                    p.kv8_sb,
                    p.kvs_sb,
                    C,
                    p.H,
                    IND ? p.src + b * p.src_ld : nullptr,
                    (int)gridDim.y - 1,
                    0,
                    0,
                    nw,
                    mine8 + tc * 2 * C,
                    mines + tc * 2 * p.H,
                    &own};
  if constexpr (GAP) {
    kv.ghi = p.gap_hi;
    kv.glo = min(max((int64_t)p.gap_lo[b], (int64_t)0), kv.ghi);
  }
  attn_decode_body(nw, p.scale, tc + 1, kv, p.o + b * p.o_ld + h * 64);
}

template <bool IND, bool GAP>
int launch_q8(const Q8P& p, int64_t R, gvl_stream_t stream) {
  hipLaunchKernelGGL((attn_decode_q8_kernel<IND, GAP>), dim3((unsigned)p.H, (unsigned)R),
                     dim3(DEC_NT), 0, gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK("gvl_attn_decode_q8");
  return 0;
}

}  // namespace

extern "C" int gvl_kv_quantize_i8(const void* qkv, int64_t qkv_sb, int64_t qkv_st, void* kv8,
                                  int64_t kv8_sb, float* kvs, int64_t kvs_sb, int64_t B, int64_t S,
                                  int64_t H, int64_t col0, gvl_stream_t stream) {
  GVL_REQUIRE(qkv && kv8 && kvs, "gvl_kv_quantize_i8: null buffer");
  GVL_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && S <= DEC_MAXT && H >= 0 && H <= 65535,
              "gvl_kv_quantize_i8: B=%lld / S=%lld / H=%lld out of range", (long long)B,
              (long long)S, (long long)H);
  GVL_REQUIRE(col0 >= 0 && col0 + S <= DEC_MAXT, "gvl_kv_quantize_i8: col0=%lld out of range",
              (long long)col0);
  GVL_REQUIRE(qkv_st >= 3 * H * 64 && (B <= 1 || qkv_sb >= S * 3 * H * 64),
              "gvl_kv_quantize_i8: qkv_st=%lld / qkv_sb=%lld are no strides of [S, 3C] rows",
              (long long)qkv_st, (long long)qkv_sb);
  GVL_REQUIRE(kv8_sb >= (col0 + S) * 2 * H * 64 && kv8_sb % 16 == 0,
              "gvl_kv_quantize_i8: kv8_sb=%lld is no stride of [col0 + S, 2C] rows",
              (long long)kv8_sb);
  GVL_REQUIRE(kvs_sb >= (col0 + S) * 2 * H,
              "gvl_kv_quantize_i8: kvs_sb=%lld is no stride of [col0 + S, 2H] rows",
              (long long)kvs_sb);
  GVL_REQUIRE(gvl::aligned16(kv8), "gvl_kv_quantize_i8: kv8 must be 16-byte aligned");
  const int64_t total = B * S * 2 * H;
  if (total == 0) return 0;
  const int64_t blocks = (total + KVQ_NT / 64 - 1) / (KVQ_NT / 64);
  GVL_REQUIRE(blocks <= 0x7fffffff, "gvl_kv_quantize_i8: B * S * H = %lld too large",
              (long long)(B * S * H));
  KvqP p{static_cast<const bf16_t*>(qkv), static_cast<int8_t*>(kv8), kvs, qkv_sb, qkv_st,
         kv8_sb, kvs_sb, S, H, col0, total};
  hipLaunchKernelGGL(kv_quantize_i8_kernel, dim3((unsigned)blocks), dim3(KVQ_NT), 0,
                     gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK("gvl_kv_quantize_i8");
  return 0;
}

extern "C" int gvl_attn_decode_q8(const void* qkv, void* kv8, int64_t kv8_sb, float* kvs,
                                  int64_t kvs_sb, int64_t Tmax, int64_t t, const int32_t* t_dev,
                                  void* o, int64_t o_ld, int64_t R, int64_t H, float scale,
                                  const int32_t* src, int64_t src_ld, const int32_t* gap_lo,
                                  int64_t gap_hi, gvl_stream_t stream) {
  GVL_REQUIRE(qkv && kv8 && kvs && o, "gvl_attn_decode_q8: null buffer");
  GVL_REQUIRE(Tmax >= 1 && Tmax <= DEC_MAXT, "gvl_attn_decode_q8: Tmax=%lld out of range (1..%d)",
              (long long)Tmax, DEC_MAXT);
  GVL_REQUIRE(R >= 0 && R <= 65535 && H >= 0 && H <= 65535,
              "gvl_attn_decode_q8: R=%lld / H=%lld out of range", (long long)R, (long long)H);
  GVL_REQUIRE(kv8_sb >= Tmax * 2 * H * 64 && kv8_sb % 16 == 0,
              "gvl_attn_decode_q8: kv8_sb=%lld is no stride of [Tmax, 2C] rows",
              (long long)kv8_sb);
  GVL_REQUIRE(kvs_sb >= Tmax * 2 * H,
              "gvl_attn_decode_q8: kvs_sb=%lld is no stride of [Tmax, 2H] rows",
              (long long)kvs_sb);
  GVL_REQUIRE(o_ld >= H * 64, "gvl_attn_decode_q8: o_ld=%lld < C", (long long)o_ld);
  GVL_REQUIRE(gvl::aligned16(qkv) && gvl::aligned16(kv8),
              "gvl_attn_decode_q8: qkv and kv8 must be 16-byte aligned");
  GVL_REQUIRE(!src || src_ld >= Tmax, "gvl_attn_decode_q8: src_ld=%lld < Tmax=%lld",
              (long long)src_ld, (long long)Tmax);
  GVL_REQUIRE(!gap_lo || (gap_hi >= 0 && gap_hi <= Tmax),
              "gvl_attn_decode_q8: gap_hi=%lld outside 0..Tmax=%lld", (long long)gap_hi,
              (long long)Tmax);
  if (R == 0 || H == 0) return 0;
  // (a host column outside the cache is the device's: a no-op)
  if (!t_dev && (t < 0 || t >= Tmax)) return 0;
  Q8P p{static_cast<const bf16_t*>(qkv), static_cast<int8_t*>(kv8), kvs, static_cast<bf16_t*>(o),
        t_dev, t, kv8_sb, kvs_sb, o_ld, Tmax, H, scale, src, src ? src_ld : 0, gap_lo,
        gap_lo ? gap_hi : 0};
  if (gap_lo) return src ? launch_q8<true, true>(p, R, stream) : launch_q8<false, true>(p, R, stream);
  return src ? launch_q8<true, false>(p, R, stream) : launch_q8<false, false>(p, R, stream);
}
