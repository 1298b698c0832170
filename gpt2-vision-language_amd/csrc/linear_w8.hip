// Int8 weight-only decoding (include/gvl.h gvl_quantize_rows_i8, gvl_dequantize_rows_i8,
// gvl_linear_w8): per-row symmetric int8 weights with one fp32 scale per output row, and the
// linear kernel for a few rows of x that streams them.
//
// linear_w8_kernel<I8, MT>: one 512-thread workgroup per 16 output columns (16 rows of w) and per
// pass of 64 rows of x; MT = 16-row tiles of x per pass (1, 2 or 4).  The weight is the MFMA's A
// operand, x its B operand, so lane l ends up with row m = l & 15 of x and the 4 columns
// n0 + 4 (l >> 4) .. + 3: the layout of gemm_common.h's epilogue quads.
//   * K is cut into 64-wide chunks, chunk c goes to wave c % 8.  Nothing is shared between
//     waves, so every operand goes global -> VGPR (no LDS round trip): per chunk a lane loads 16
//     bytes of its weight row (int8: k0 + 16 g .. + 15, g = l >> 4; bf16: twice 16 bytes) and,
//     per tile of x, the same 16 k of its x row.  The 16 k of a lane feed two 32-deep MFMA
//     steps, 8 each: k is permuted inside the chunk, identically in both operands
//     (gemm_w4d.h's trick), which changes no product, only which MFMA adds it.
//   * int8 -> bf16 is exact (|q| <= 127); the int8 instance differs from the bf16 one only in
//     that conversion and in the fp32 multiply by scale[n] in front of the epilogue.
//   * the 8 waves' fp32 partials go through LDS and are added in wave order by the wave that
//     runs the tile's epilogue.  Waves without a chunk add zeros: the order is a function of K
//     alone.  An element's bits therefore depend on its x row, its w row, its scale and its
//     epilogue operands only (not on M, MT, the pass, ldc or the grid).
//   * rows past M and w rows past N are clamped for the loads (a clamped row only feeds MFMA
//     columns / rows whose results are never stored) and masked for the stores.
// The epilogue's fp32 operations are written with the non-contracting intrinsics so that every
// instance rounds alike: scale, +bias, tanh-GELU, *tanh(gate), +residual, one bf16 rounding.
#include "common.h"
#include "capi_util.h"
#include "../../include/gvl.h"

namespace {

constexpr int W8_WAVES = 8;
constexpr int W8_NT = 64 * W8_WAVES;
constexpr int W8_U = 4;  // chunks per group of weight loads

struct W8P {
  const bf16_t* x;
  const void* w;
  const float* scale;
  bf16_t* c;
  int64_t M, N, K, ldx, ldw, ldc, ldr;
  const bf16_t* bias;
  const bf16_t* residual;
  const bf16_t* gate;
  int act;
};

// 8 int8 (two dwords) -> 8 bf16, exact: sign-extend, convert, keep the upper half
GVL_DEV uint32_t cvt2(uint32_t d, int b) {
  const float lo = (float)(int)(int8_t)(d >> (8 * b));
  const float hi = (float)(int)(int8_t)(d >> (8 * b + 8));
  return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}
GVL_DEV short8_t cvt8(uint32_t d0, uint32_t d1) {
  const uint4 u = make_uint4(cvt2(d0, 0), cvt2(d0, 2), cvt2(d1, 0), cvt2(d1, 2));
  return __builtin_bit_cast(short8_t, u);
}

template <bool I8, int MT>
__global__ __launch_bounds__(W8_NT) void linear_w8_kernel(const W8P p) {
  __shared__ float4_t red[W8_WAVES][MT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int64_t n0 = (int64_t)blockIdx.x * 16, m0 = (int64_t)blockIdx.y * 64;
  int64_t nrow = n0 + i;
  nrow = nrow < p.N ? nrow : p.N - 1;
  constexpr int WB = I8 ? 1 : 2;  // bytes per weight
  const char* wp = reinterpret_cast<const char*>(p.w) + (nrow * p.ldw + 16 * g) * WB;
  const bf16_t* xp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    int64_t m = m0 + 16 * t + i;
    m = m < p.M ? m : p.M - 1;
    xp[t] = p.x + m * p.ldx + 16 * g;
  }
  float4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = float4_t{0.f, 0.f, 0.f, 0.f};

  // This wave's chunks: wave, wave + 8, ...  The weight fragments of W8_U chunks are loaded
  // together and the next W8_U are issued before the current ones are used (the HBM stream
  // stays 2 * W8_U loads deep per lane); a group reaching past the wave's last chunk re-loads
  // that chunk (no branch around a load) and skips its MFMAs.
  const int nchunk = (int)(p.K >> 6);
  const int it = (nchunk - wave + W8_WAVES - 1) / W8_WAVES;
  constexpr int NW = I8 ? 1 : 2;  // 16-byte loads per weight fragment
  uint4 cur[W8_U][NW], nxt[W8_U][NW];
  auto wload = [&](uint4 (&f)[W8_U][NW], int j) {
#pragma unroll
    for (int u = 0; u < W8_U; ++u) {
      const int jj = j + u < it ? j + u : it - 1;
      const char* src = wp + (int64_t)(wave + W8_WAVES * jj) * 64 * WB;
#pragma unroll
      for (int h = 0; h < NW; ++h) f[u][h] = *reinterpret_cast<const uint4*>(src + 16 * h);
    }
  };
  if (it > 0) wload(cur, 0);
  for (int j = 0; j < it; j += W8_U) {
    if (j + W8_U < it) wload(nxt, j + W8_U);
#pragma unroll
    for (int u = 0; u < W8_U; ++u) {
      if (j + u < it) {
        const int64_t k0 = (int64_t)(wave + W8_WAVES * (j + u)) * 64;
        short8_t a0, a1;
        if constexpr (I8) {
          a0 = cvt8(cur[u][0].x, cur[u][0].y);
          a1 = cvt8(cur[u][0].z, cur[u][0].w);
        } else {
          a0 = __builtin_bit_cast(short8_t, cur[u][0]);
          a1 = __builtin_bit_cast(short8_t, cur[u][NW - 1]);
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const short8_t b0 =
              __builtin_bit_cast(short8_t, *reinterpret_cast<const uint4*>(xp[t] + k0));
          const short8_t b1 =
              __builtin_bit_cast(short8_t, *reinterpret_cast<const uint4*>(xp[t] + k0 + 8));
          acc[t] = mfma16(a0, b0, acc[t]);
          acc[t] = mfma16(a1, b1, acc[t]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < W8_U; ++u)
#pragma unroll
      for (int h = 0; h < NW; ++h) cur[u][h] = nxt[u][h];
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave >= MT) return;

  // wave t: tile t's sum in wave order, then its epilogue
  const int t = wave;
  float4_t s = red[0][t][lane];
#pragma unroll
  for (int w = 1; w < W8_WAVES; ++w) {
    const float4_t r = red[w][t][lane];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = __fadd_rn(s[e], r[e]);
  }
  const int64_t m = m0 + 16 * t + i, n = n0 + 4 * g;
  if (m >= p.M || n >= p.N) return;
  float v[4] = {s[0], s[1], s[2], s[3]};
  if constexpr (I8) {
    const float4 sc = *reinterpret_cast<const float4*>(p.scale + n);
    v[0] = __fmul_rn(v[0], sc.x); v[1] = __fmul_rn(v[1], sc.y);
    v[2] = __fmul_rn(v[2], sc.z); v[3] = __fmul_rn(v[3], sc.w);
  }
  if (p.bias) {
    const uint2 bb = *reinterpret_cast<const uint2*>(p.bias + n);
    v[0] = __fadd_rn(v[0], lo_bf(bb.x)); v[1] = __fadd_rn(v[1], hi_bf(bb.x));
    v[2] = __fadd_rn(v[2], lo_bf(bb.y)); v[3] = __fadd_rn(v[3], hi_bf(bb.y));
  }
  if (p.act) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
  }
  if (p.gate) {
    const float gatev = tanhf(bf2f(*p.gate));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __fmul_rn(v[e], gatev);
  }
  if (p.residual) {
    const uint2 rr = *reinterpret_cast<const uint2*>(p.residual + m * p.ldr + n);
    v[0] = __fadd_rn(v[0], lo_bf(rr.x)); v[1] = __fadd_rn(v[1], hi_bf(rr.x));
    v[2] = __fadd_rn(v[2], lo_bf(rr.y)); v[3] = __fadd_rn(v[3], hi_bf(rr.y));
  }
  *reinterpret_cast<uint2*>(p.c + m * p.ldc + n) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
}

template <bool I8>
void w8_launch(const W8P& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.N + 15) / 16), (unsigned)((p.M + 63) / 64));
  if (p.M <= 16) hipLaunchKernelGGL((linear_w8_kernel<I8, 1>), grid, dim3(W8_NT), 0, s, p);
  else if (p.M <= 32) hipLaunchKernelGGL((linear_w8_kernel<I8, 2>), grid, dim3(W8_NT), 0, s, p);
  else hipLaunchKernelGGL((linear_w8_kernel<I8, 4>), grid, dim3(W8_NT), 0, s, p);
}

// ---------------------------------------------------------------- quantiser / dequantiser
constexpr int Q_NT = 256;

// One workgroup per row: the row's absmax over the bf16 magnitudes compared as integers (so a
// NaN or an infinity wins and reaches the scale), then the row again (from L2) for the values.
__global__ __launch_bounds__(Q_NT) void quantize_rows_i8_kernel(const bf16_t* w, int64_t ldw,
                                                                int64_t K, int8_t* q, int64_t ldq,
                                                                float* scale) {
  __shared__ uint32_t red[Q_NT / 64];
  const int64_t n = blockIdx.x;
  const bf16_t* row = w + n * ldw;
  uint32_t mx = 0;
  for (int64_t k = 8 * (int64_t)threadIdx.x; k < K; k += 8 * Q_NT) {
    const uint4 u = *reinterpret_cast<const uint4*>(row + k);
    const uint32_t d[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t lo = d[e] & 0x7fffu, hi = (d[e] >> 16) & 0x7fffu;
      mx = mx > lo ? mx : lo;
      mx = mx > hi ? mx : hi;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, 64);
    mx = mx > other ? mx : other;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < Q_NT / 64; ++e) mx = mx > red[e] ? mx : red[e];
  const float s = __fdiv_rn(bf2f(mx), 127.f);
  if (threadIdx.x == 0) scale[n] = s;
  int8_t* qrow = q + n * ldq;
  for (int64_t k = 8 * (int64_t)threadIdx.x; k < K; k += 8 * Q_NT) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(row + k), f);
    uint32_t o[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float r = 0.f;
      if (mx != 0u) r = fminf(fmaxf(rintf(__fdiv_rn(f[e], s)), -127.f), 127.f);
      o[e >> 2] |= ((uint32_t)(int)r & 0xffu) << (8 * (e & 3));
    }
    *reinterpret_cast<uint2*>(qrow + k) = make_uint2(o[0], o[1]);
  }
}

__global__ __launch_bounds__(Q_NT) void dequantize_rows_i8_kernel(const int8_t* q, int64_t ldq,
                                                                  const float* scale, int64_t K,
                                                                  bf16_t* out, int64_t ldo) {
  const int64_t n = blockIdx.x;
  const float s = scale[n];
  for (int64_t k = 8 * (int64_t)threadIdx.x; k < K; k += 8 * Q_NT) {
    const uint2 u = *reinterpret_cast<const uint2*>(q + n * ldq + k);
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      f[e] = __fmul_rn((float)(int)(int8_t)((e < 4 ? u.x : u.y) >> (8 * (e & 3))), s);
    *reinterpret_cast<uint4*>(out + n * ldo + k) = pack8(f);
  }
}

}  // namespace

extern "C" int gvl_quantize_rows_i8(const void* w, int64_t ldw, int64_t n, int64_t k, void* q,
                                    int64_t ldq, float* scale, gvl_stream_t stream) {
  GVL_REQUIRE(w && q && scale, "gvl_quantize_rows_i8: null operand");
  GVL_REQUIRE(n >= 1 && n <= 0x7fffffff && k >= 8 && k % 8 == 0 && ldw >= k && ldq >= k &&
                  ldw % 8 == 0 && ldq % 8 == 0,
              "gvl_quantize_rows_i8: shape unsupported (N=%lld K=%lld ldw=%lld ldq=%lld; K, ldw, "
              "ldq multiples of 8)", (long long)n, (long long)k, (long long)ldw, (long long)ldq);
  GVL_REQUIRE(gvl::aligned16(w) && gvl::aligned16(q) && gvl::aligned16(scale),
              "gvl_quantize_rows_i8: operands must be 16-byte aligned");
  hipLaunchKernelGGL(quantize_rows_i8_kernel, dim3((unsigned)n), dim3(Q_NT), 0,
                     gvl::as_stream(stream), reinterpret_cast<const bf16_t*>(w), ldw, k,
                     reinterpret_cast<int8_t*>(q), ldq, scale);
  GVL_LAUNCH_CHECK("gvl_quantize_rows_i8");
  return 0;
}

extern "C" int gvl_dequantize_rows_i8(const void* q, int64_t ldq, const float* scale, int64_t n,
                                      int64_t k, void* out, int64_t ldo, gvl_stream_t stream) {
  GVL_REQUIRE(q && scale && out, "gvl_dequantize_rows_i8: null operand");
  GVL_REQUIRE(n >= 1 && n <= 0x7fffffff && k >= 8 && k % 8 == 0 && ldq >= k && ldo >= k &&
                  ldq % 8 == 0 && ldo % 8 == 0,
              "gvl_dequantize_rows_i8: shape unsupported (N=%lld K=%lld ldq=%lld ldo=%lld; K, "
              "ldq, ldo multiples of 8)", (long long)n, (long long)k, (long long)ldq,
              (long long)ldo);
  GVL_REQUIRE(gvl::aligned16(q) && gvl::aligned16(scale) && gvl::aligned16(out),
              "gvl_dequantize_rows_i8: operands must be 16-byte aligned");
  hipLaunchKernelGGL(dequantize_rows_i8_kernel, dim3((unsigned)n), dim3(Q_NT), 0,
                     gvl::as_stream(stream), reinterpret_cast<const int8_t*>(q), ldq, scale, k,
                     reinterpret_cast<bf16_t*>(out), ldo);
  GVL_LAUNCH_CHECK("gvl_dequantize_rows_i8");
  return 0;
}

extern "C" int gvl_linear_w8(const gvl_linear_w8_desc* d, gvl_stream_t stream) {
  GVL_REQUIRE(d != nullptr, "gvl_linear_w8: null descriptor");
  GVL_REQUIRE(d->x && d->w && d->c, "gvl_linear_w8: null operand");
  const bool i8 = d->scale != nullptr;
  GVL_REQUIRE(d->k >= 64 && d->k % 64 == 0, "gvl_linear_w8: K must be a multiple of 64 (K=%lld)",
              (long long)d->k);
  GVL_REQUIRE(d->n >= 8 && d->n % 8 == 0 && d->n <= (int64_t)16 * 0x7fffffff,
              "gvl_linear_w8: N must be a multiple of 8 (N=%lld)", (long long)d->n);
  GVL_REQUIRE(d->m >= 1 && d->m <= GVL_LINEAR_W8_MAX_ROWS,
              "gvl_linear_w8: M=%lld outside 1..%d rows", (long long)d->m,
              GVL_LINEAR_W8_MAX_ROWS);
  const bool bias = d->bias != nullptr, res = d->residual != nullptr, gate = d->gate != nullptr;
  const bool epi_ok = (d->act == 0 || d->act == 1) &&
                      ((!bias && !d->act && !res && !gate) ||  // plain
                       (bias && !res && !gate) ||              // bias, bias + gelu
                       (bias && !d->act && res));              // bias + residual (+ gate)
  GVL_REQUIRE(epi_ok,
              "gvl_linear_w8: unsupported epilogue (plain, bias, bias + act 1, bias + residual, "
              "bias + gate + residual)");
  GVL_REQUIRE(d->ldx >= d->k && d->ldx % 8 == 0 && d->ldw >= d->k &&
                  d->ldw % (i8 ? 16 : 8) == 0 && d->ldc >= d->n && d->ldc % 4 == 0 &&
                  (!res || (d->ldr >= d->n && d->ldr % 4 == 0)),
              "gvl_linear_w8: bad leading dimension (ldx=%lld %% 8, ldw=%lld %% %d, ldc=%lld "
              "%% 4, ldr=%lld %% 4)", (long long)d->ldx, (long long)d->ldw, i8 ? 16 : 8,
              (long long)d->ldc, (long long)d->ldr);
  GVL_REQUIRE(gvl::aligned16(d->x) && gvl::aligned16(d->w) && gvl::aligned16(d->c) &&
                  gvl::aligned16(d->scale) && gvl::aligned16(d->bias) &&
                  gvl::aligned16(d->residual),
              "gvl_linear_w8: operands must be 16-byte aligned");
  W8P p{reinterpret_cast<const bf16_t*>(d->x), d->w, d->scale, reinterpret_cast<bf16_t*>(d->c),
        d->m, d->n, d->k, d->ldx, d->ldw, d->ldc, d->ldr,
        reinterpret_cast<const bf16_t*>(d->bias), reinterpret_cast<const bf16_t*>(d->residual),
        reinterpret_cast<const bf16_t*>(d->gate), d->act};
  if (i8) w8_launch<true>(p, gvl::as_stream(stream));
  else w8_launch<false>(p, gvl::as_stream(stream));
  GVL_LAUNCH_CHECK("gvl_linear_w8");
  return 0;
}
