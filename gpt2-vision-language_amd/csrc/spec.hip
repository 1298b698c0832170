// Speculative decoding (include/gvl.h): verify a few drafted tokens per sequence in one
// KV-cached decoder pass.  Three latency-bound kernels.
//
// attn_decode_multi_kernel: Q new queries per sequence at per-sequence cache lengths, the K/V
// append fused.  One 256-thread workgroup per (head, sequence, query), the query on gridDim.z.
// It runs attn_decode_body (attn_decode.h) with the append policy: position t < kv_len comes
// from the cache, position t >= kv_len from row t - kv_len of this step's c_attn output, and
// the workgroup of query j copies its head's k and v of row j into cache[kv_len + j] before
// the first barrier.  Every load of the cache in the launch is at a position below kv_len and
// every store at or past it, so the append races with no load.
//
// ngram_draft_kernel: one 256-thread workgroup per sequence; the sequence (prompt + emitted
// tokens, <= 4096) sits in LDS and every thread tests candidate starts for the longest suffix
// first ("prompt lookup").
//
// spec_accept_kernel: one thread per sequence compares the chosen tokens with the draft and
// advances the per-sequence state on the device.
#include "attn_decode.h"
#include "capi_util.h"
#include "../../include/gvl.h"

namespace {

constexpr int SPD_MAXQ = 8;

struct MultiP {
  const bf16_t* qkv;  // [B, Q, 3C] contiguous
  bf16_t* cache;      // [B, Tmax, 3C], rows 3C apart, sequences cache_sb apart
  bf16_t* o;          // [B*Q, C], rows o_ld apart
  const int32_t* kv_len;
  int64_t cache_sb, o_ld, Tmax, C;
  int Q;
  float scale;
};

// The KV policy (attn_decode.h) of query jq of a sequence with `len` cached positions: position
// t < len is row t of the cache, position t >= len is row t - len of this step's qkv.
struct AppendKV : BF16Elems<AppendKV> {
  static constexpr bool may_be_empty = false;  // a query always attends itself
  bf16_t* cb;        // the sequence's cache rows
  const bf16_t* nw;  // this step's rows of the sequence
  int64_t len, C3, koff, voff;  // the head's k / v columns within a row
  int jq;
  GVL_DEV void prologue(int tid) const {  // append: 8 x 16 B of k, 8 x 16 B of v
    if (tid >= 64 && tid < 80) {
      const int c = tid - 64;
      const int64_t off = (c < 8 ? koff : voff) + (c & 7) * 8;
      *reinterpret_cast<uint4*>(cb + (len + jq) * C3 + off) =
          *reinterpret_cast<const uint4*>(nw + jq * C3 + off);
    }
  }
  GVL_DEV bool skip(int64_t) const { return false; }
  GVL_DEV const bf16_t* row(int64_t t) const {
    return t < len ? cb + t * C3 : nw + (t - len) * C3;
  }
  GVL_DEV const bf16_t* key(int64_t t) const { return row(t) + koff; }
  GVL_DEV const bf16_t* value(int64_t t) const { return row(t) + voff; }
};

__global__ __launch_bounds__(DEC_NT) void attn_decode_multi_kernel(MultiP p) {
  const int h = blockIdx.x, b = blockIdx.y, jq = blockIdx.z;
  const int64_t C3 = 3 * p.C;
  // the cached length, clamped so that neither the append nor sc[] can leave its array
  const int64_t lmax = min(p.Tmax, (int64_t)DEC_MAXT) - p.Q;
  const int64_t len = min(max((int64_t)p.kv_len[b], (int64_t)0), lmax);
  const bf16_t* nw = p.qkv + (int64_t)b * p.Q * C3;
  const AppendKV kv{{}, p.cache + b * p.cache_sb, nw, len, C3, p.C + h * 64, 2 * p.C + h * 64, jq};
  attn_decode_body(nw + jq * C3 + h * 64, p.scale, len + jq + 1, kv,
                   p.o + ((int64_t)b * p.Q + jq) * p.o_ld + h * 64);
}

struct DraftP {
  const int64_t* prompt;
  const int32_t* plen;
  const int64_t* emitted;
  const int32_t* n;
  const int64_t* given;
  int64_t* draft;
  int64_t prompt_ld, emitted_ld, given_ld;
  int P, n_new, ngram, D;
};

GVL_DEV int32_t id32(int64_t v) {  // ids are compared as int32; one outside it saturates
  return (int32_t)min(max(v, (int64_t)INT32_MIN), (int64_t)INT32_MAX);
}

__global__ __launch_bounds__(DEC_NT) void ngram_draft_kernel(DraftP p) {
  __shared__ int32_t s[DEC_MAXT];
  __shared__ int best;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int pl = min(max(p.plen[b], 0), p.P);
  const int nb = min(max(p.n[b], 0), p.n_new);
  const int L = pl + nb;  // <= P + n_new <= DEC_MAXT (host check)
  const bool live = nb < p.n_new;
  for (int t = tid; t < L; t += DEC_NT)
    s[t] = id32(t < pl ? p.prompt[b * p.prompt_ld + t] : p.emitted[b * p.emitted_ld + t - pl]);
  int at = -1;  // where the continuation starts: i + g of the winning match
  for (int g = p.ngram; g >= 1 && live; --g) {  // (block-uniform conditions)
    __syncthreads();
    if (tid == 0) best = -1;
    __syncthreads();
    if (g > L - 1) continue;
    int mine = -1;
    for (int i = tid; i + g <= L - 1; i += DEC_NT) {
      bool eq = true;
      for (int c = 0; c < g; ++c) eq = eq && s[i + c] == s[L - g + c];
      if (eq) mine = i;  // i grows: the thread keeps its largest
    }
    if (mine >= 0) atomicMax(&best, mine);
    __syncthreads();
    if (best >= 0) {
      at = best + g;
      break;
    }
  }
  if (tid < p.D) {
    int64_t d = -1;
    if (live) {
      if (at >= 0 && at + tid < L) d = s[at + tid];
      if (p.given && nb + tid < p.n_new) {
        const int64_t gv = p.given[b * p.given_ld + nb + tid];
        if (gv >= 0) d = gv;
      }
    }
    p.draft[(int64_t)b * p.D + tid] = d;
  }
}

struct AcceptP {
  const int64_t* x;
  const int64_t* draft;
  int32_t* n;
  int32_t* kv_len;
  int32_t* pos;
  int32_t* lengths;
  int64_t* last;
  int64_t* out;
  int32_t* drafted;
  int32_t* accepted;
  int64_t out_ld, eos, B;
  int Q, n_new;
};

__global__ void spec_accept_kernel(AcceptP p) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  const int nb = p.n[b];
  if (nb < 0 || nb >= p.n_new) return;  // finished: every bit of its state stays
  const int64_t* x = p.x + b * p.Q;
  const int64_t* dr = p.draft ? p.draft + b * (p.Q - 1) : nullptr;
  int a = 0, guesses = 0;
  bool run = true;
  for (int j = 0; j < p.Q - 1; ++j) {
    const int64_t d = dr[j];
    guesses += d >= 0;
    run = run && d == x[j];
    a += run;
  }
  int m = min(a + 1, p.n_new - nb);
  bool ended = false;
  if (p.eos >= 0)
    for (int e = 0; e < m; ++e)
      if (x[e] == p.eos) {
        m = e + 1;
        ended = true;
        break;
      }
  int64_t* o = p.out + b * p.out_ld;
  for (int j = 0; j < m; ++j) o[nb + j] = x[j];
  if (ended) {
    p.lengths[b] = nb + m;
    for (int t = nb + m; t < p.n_new; ++t) o[t] = p.eos;
    p.n[b] = p.n_new;
  } else {
    p.n[b] = nb + m;
  }
  p.kv_len[b] += m;
  p.pos[b] += m;
  p.last[b] = x[m - 1];
  if (p.drafted) p.drafted[b] += guesses;
  if (p.accepted) p.accepted[b] += m - 1;
}

}  // namespace

extern "C" int gvl_attn_decode_multi(const void* qkv, void* cache, int64_t cache_sb, int64_t Tmax,
                                     const int32_t* kv_len, void* o, int64_t o_ld, int64_t B,
                                     int64_t H, int64_t Q, float scale, gvl_stream_t stream) {
  GVL_REQUIRE(qkv && cache && o, "gvl_attn_decode_multi: null buffer");
  GVL_REQUIRE(kv_len, "gvl_attn_decode_multi: null kv_len");
  GVL_REQUIRE(Q >= 1 && Q <= SPD_MAXQ, "gvl_attn_decode_multi: Q=%lld out of range (1..%d)",
              (long long)Q, SPD_MAXQ);
  GVL_REQUIRE(B >= 0 && B <= 65535 && H >= 0 && H <= 65535,
              "gvl_attn_decode_multi: B=%lld / H=%lld out of range", (long long)B, (long long)H);
  GVL_REQUIRE(Tmax >= Q, "gvl_attn_decode_multi: Tmax=%lld < Q=%lld", (long long)Tmax,
              (long long)Q);
  GVL_REQUIRE(cache_sb >= Tmax * 3 * H * 64 && cache_sb % 8 == 0,
              "gvl_attn_decode_multi: cache_sb=%lld is no stride of [Tmax, 3C] rows",
              (long long)cache_sb);
  GVL_REQUIRE(o_ld >= H * 64, "gvl_attn_decode_multi: o_ld=%lld < C", (long long)o_ld);
  GVL_REQUIRE(gvl::aligned16(qkv) && gvl::aligned16(cache),
              "gvl_attn_decode_multi: qkv and cache must be 16-byte aligned");
  if (B == 0 || H == 0) return 0;
  MultiP p{static_cast<const bf16_t*>(qkv), static_cast<bf16_t*>(cache), static_cast<bf16_t*>(o),
           kv_len, cache_sb, o_ld, Tmax, H * 64, (int)Q, scale};
  hipLaunchKernelGGL(attn_decode_multi_kernel, dim3((unsigned)H, (unsigned)B, (unsigned)Q),
                     dim3(DEC_NT), 0, gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK("gvl_attn_decode_multi");
  return 0;
}

extern "C" int gvl_ngram_draft(const int64_t* prompt, int64_t prompt_ld, int64_t P,
                               const int32_t* plen, const int64_t* emitted, int64_t emitted_ld,
                               const int32_t* n, int64_t n_new, const int64_t* given,
                               int64_t given_ld, int64_t B, int32_t ngram, int32_t D,
                               int64_t* draft, gvl_stream_t stream) {
  GVL_REQUIRE(plen && emitted && n && draft, "gvl_ngram_draft: null buffer");
  GVL_REQUIRE(P >= 0 && (P == 0 || prompt) && prompt_ld >= P,
              "gvl_ngram_draft: P=%lld / prompt_ld=%lld / null prompt", (long long)P,
              (long long)prompt_ld);
  GVL_REQUIRE(n_new >= 1 && emitted_ld >= n_new && (!given || given_ld >= n_new),
              "gvl_ngram_draft: n_new=%lld, emitted_ld=%lld, given_ld=%lld", (long long)n_new,
              (long long)emitted_ld, (long long)given_ld);
  GVL_REQUIRE(P + n_new <= DEC_MAXT, "gvl_ngram_draft: P + n_new = %lld exceeds %d",
              (long long)(P + n_new), DEC_MAXT);
  GVL_REQUIRE(ngram >= 1 && ngram <= 4, "gvl_ngram_draft: ngram=%d out of range (1..4)", ngram);
  GVL_REQUIRE(D >= 1 && D <= SPD_MAXQ - 1, "gvl_ngram_draft: D=%d out of range (1..%d)", D,
              SPD_MAXQ - 1);
  GVL_REQUIRE(B >= 0 && B <= 0x7fffffff, "gvl_ngram_draft: B=%lld out of range", (long long)B);
  if (B == 0) return 0;
  DraftP p{prompt, plen, emitted, n, given, draft, prompt_ld, emitted_ld, given ? given_ld : 0,
           (int)P, (int)n_new, ngram, D};
  hipLaunchKernelGGL(ngram_draft_kernel, dim3((unsigned)B), dim3(DEC_NT), 0,
                     gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK("gvl_ngram_draft");
  return 0;
}

extern "C" int gvl_spec_accept(const int64_t* x, const int64_t* draft, int64_t B, int32_t Q,
                               int32_t* n, int32_t* kv_len, int32_t* pos, int32_t* lengths,
                               int64_t* last, int64_t* out, int64_t out_ld, int64_t n_new,
                               int64_t eos, int32_t* drafted, int32_t* accepted,
                               gvl_stream_t stream) {
  GVL_REQUIRE(x && n && kv_len && pos && lengths && last && out, "gvl_spec_accept: null buffer");
  GVL_REQUIRE(Q >= 1 && Q <= SPD_MAXQ, "gvl_spec_accept: Q=%d out of range (1..%d)", Q, SPD_MAXQ);
  GVL_REQUIRE(Q == 1 || draft, "gvl_spec_accept: null draft with Q=%d", Q);
  GVL_REQUIRE(n_new >= 1 && n_new <= 0x7fffffff && out_ld >= n_new,
              "gvl_spec_accept: n_new=%lld / out_ld=%lld", (long long)n_new, (long long)out_ld);
  GVL_REQUIRE(B >= 0 && B <= 0x7fffffff, "gvl_spec_accept: B=%lld out of range", (long long)B);
  if (B == 0) return 0;
  AcceptP p{x, draft, n, kv_len, pos, lengths, last, out, drafted, accepted, out_ld,
            eos < 0 ? -1 : eos, B, Q, (int)n_new};
  hipLaunchKernelGGL(spec_accept_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0,
                     gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK("gvl_spec_accept");
  return 0;
}
