// Logits processors between the decoder step and the token choice (include/gvl.h
// gvl_logits_process): repetition penalty, no-repeat n-gram, end-token and bad-token bans, edited
// in place on the few logits they concern.
//
// logits_process_kernel: one 256-thread workgroup per row.  The row's token sequence s (prompt,
// then the generated tokens read through the beam indirection table) is staged in LDS as int32
// (<= 4096 entries, 16 KiB).  The penalty must hit a token once however often it occurs: a V-bit
// LDS bitmap (8 KiB at V = 65536) is set by atomic-or, and only the thread that found the bit
// clear rescales that logit.  A barrier separates the penalty from the bans, so a ban always lands
// after the penalty's store to the same logit; several threads banning one logit all store -inf.
// The n-gram rule gives one candidate window per thread: n - 1 LDS compares against the tail.
// O(L + n_bad) logits touched per row; latency-bound, nothing V-wide.
#include <math.h>

#include "common.h"
#include "capi_util.h"
#include "../../include/gvl.h"

namespace {

constexpr int LP_NT = 256;
constexpr int LP_MAXL = 4096;
constexpr int LP_MAXV = 65536;
constexpr int LP_MAXN = 16;

struct LogitsP {
  void* logits;
  int64_t ld, R, V;
  int f32;
  const int64_t* hist;
  int64_t hist_ld;
  int n_hist;
  const int32_t* src;
  int64_t src_ld, t0;
  const int64_t* prompt;
  int64_t prompt_ld;
  int P, rows_per_item;
  float pen;
  int ngram, eos, ban_eos;
  const int32_t* bad;
  int n_bad;
  const int32_t* flen;
};

// a token id as the int32 the kernel compares: ids past int32 saturate, so none of them can
// alias an id inside the vocabulary
GVL_DEV int32_t tok32(int64_t v) {
  return v < INT32_MIN ? INT32_MIN : v > INT32_MAX ? INT32_MAX : (int32_t)v;
}

GVL_DEV void ban(const LogitsP& p, int64_t row, int32_t v) {
  if (v < 0 || v >= p.V) return;
  if (p.f32) reinterpret_cast<float*>(p.logits)[row * p.ld + v] = -INFINITY;
  else reinterpret_cast<bf16_t*>(p.logits)[row * p.ld + v] = 0xFF80u;  // bf16 -inf
}

// The one body of both kernels: n_hist and ban_eos come from the launch arguments
// (logits_process_kernel) or from a step count in device memory (logits_process_dev_kernel).
GVL_DEV void logits_process_body(const LogitsP& p, int n_hist, bool ban_eos) {
  __shared__ int32_t s[LP_MAXL];
  __shared__ uint32_t seen[LP_MAXV / 32];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (p.flen != nullptr && p.flen[row] > 0) return;  // (block-uniform) a finished beam
  const int L = p.P + n_hist;
  const bool pen = p.pen != 1.f;
  const int64_t item = row / p.rows_per_item;
  for (int i = tid; i < L; i += LP_NT) {
    int64_t v;
    if (i < p.P) {
      v = p.prompt[item * p.prompt_ld + i];
    } else {
      const int g = i - p.P;
      int64_t hr = row;
      if (p.src != nullptr) {
        hr = p.src[row * p.src_ld + p.t0 + g];
        hr = hr < 0 ? 0 : hr >= p.R ? p.R - 1 : hr;
      }
      v = p.hist[(int64_t)g * p.hist_ld + hr];
    }
    s[i] = tok32(v);
  }
  if (pen)
    for (int w = tid; w < (int)((p.V + 31) >> 5); w += LP_NT) seen[w] = 0u;
  __syncthreads();

  if (pen) {
    for (int i = tid; i < L; i += LP_NT) {
      const int32_t v = s[i];
      if (v < 0 || v >= p.V) continue;
      const uint32_t bit = 1u << (v & 31);
      if (atomicOr(&seen[v >> 5], bit) & bit) continue;  // another occurrence took it
      if (p.f32) {
        float* q = reinterpret_cast<float*>(p.logits) + row * p.ld + v;
        const float x = *q;
        *q = x < 0.f ? x * p.pen : x / p.pen;
      } else {
        bf16_t* q = reinterpret_cast<bf16_t*>(p.logits) + row * p.ld + v;
        const float x = bf2f(*q);
        *q = f2bf(x < 0.f ? x * p.pen : x / p.pen);
      }
    }
    __syncthreads();  // every ban below lands after the penalty's store to the same logit
  }

  const int n = p.ngram;
  if (n == 1) {
    for (int i = tid; i < L; i += LP_NT) ban(p, row, s[i]);
  } else if (n >= 2 && L >= n) {
    const int tail = L - n + 1;  // the last n - 1 tokens: s[tail .. L)
    for (int i = tid; i <= L - n; i += LP_NT) {
      bool same = true;
      for (int j = 0; j < n - 1; ++j) same = same && s[i + j] == s[tail + j];
      if (same) ban(p, row, s[i + n - 1]);
    }
  }
  if (tid == 0 && ban_eos) ban(p, row, p.eos);
  for (int i = tid; i < p.n_bad; i += LP_NT) ban(p, row, p.bad[i]);
}

__global__ __launch_bounds__(LP_NT) void logits_process_kernel(LogitsP p) {
  logits_process_body(p, p.n_hist, p.ban_eos != 0);
}

// gvl_logits_process_dev: n_hist = clamp(*step, 0, hist_cap), eos banned while *step < min_new
// (p.n_hist and p.ban_eos go unused).
__global__ __launch_bounds__(LP_NT) void logits_process_dev_kernel(LogitsP p, const int32_t* step,
                                                                   int hist_cap, int min_new) {
  const int st = *step;
  logits_process_body(p, min(max(st, 0), hist_cap), st < min_new);
}

}  // namespace

// What both entry points require alike; fn names the caller and cnt its history count (n_hist,
// or hist_cap: the most *step can make it) in the message.
static int check_logits(const char* fn, const char* cnt, const void* logits, int64_t ld, int64_t R,
                        int64_t V, const int64_t* hist, int64_t hist_ld, int32_t n_hist,
                        const int32_t* src, int64_t src_ld, int64_t t0, const int64_t* prompt,
                        int64_t prompt_ld, int32_t P, int32_t rows_per_item, float rep_penalty,
                        int32_t ngram, const int32_t* bad, int32_t n_bad) {
  GVL_REQUIRE(logits != nullptr, "%s: null logits", fn);
  GVL_REQUIRE(V >= 1 && V <= LP_MAXV, "%s: V=%lld out of range (1..%d)", fn, (long long)V, LP_MAXV);
  GVL_REQUIRE(ld >= V, "%s: ld=%lld < V=%lld", fn, (long long)ld, (long long)V);
  GVL_REQUIRE(R >= 0 && R <= 0x7fffffff, "%s: R=%lld out of range", fn, (long long)R);
  GVL_REQUIRE(n_hist >= 0, "%s: %s=%d is negative", fn, cnt, (int)n_hist);
  GVL_REQUIRE(P >= 0, "%s: P=%d is negative", fn, (int)P);
  GVL_REQUIRE(n_bad >= 0, "%s: n_bad=%d is negative", fn, (int)n_bad);
  GVL_REQUIRE((int64_t)P + n_hist <= LP_MAXL, "%s: L = P + %s = %lld exceeds %d", fn, cnt,
              (long long)P + n_hist, LP_MAXL);
  GVL_REQUIRE(ngram >= 0 && ngram <= LP_MAXN, "%s: ngram=%d out of range (0..%d)", fn, (int)ngram,
              LP_MAXN);
  GVL_REQUIRE(isfinite(rep_penalty) && rep_penalty > 0.f,
              "%s: rep_penalty=%g must be finite and positive", fn, (double)rep_penalty);
  GVL_REQUIRE(rows_per_item >= 1 && R % rows_per_item == 0,
              "%s: rows_per_item=%d must be >= 1 and divide R=%lld", fn, (int)rows_per_item,
              (long long)R);
  GVL_REQUIRE(n_hist == 0 || hist != nullptr, "%s: null hist with %s=%d", fn, cnt, (int)n_hist);
  GVL_REQUIRE(n_hist == 0 || hist_ld >= R, "%s: hist_ld=%lld < R=%lld", fn, (long long)hist_ld,
              (long long)R);
  GVL_REQUIRE(src == nullptr || (t0 >= 0 && src_ld >= t0 + n_hist),
              "%s: src_ld=%lld does not hold t0 + %s = %lld columns (t0=%lld)", fn,
              (long long)src_ld, cnt, (long long)(t0 + n_hist), (long long)t0);
  GVL_REQUIRE(P == 0 || prompt != nullptr, "%s: null prompt with P=%d", fn, (int)P);
  GVL_REQUIRE(P == 0 || prompt_ld >= P, "%s: prompt_ld=%lld < P=%d", fn, (long long)prompt_ld,
              (int)P);
  GVL_REQUIRE(n_bad == 0 || bad != nullptr, "%s: null bad with n_bad=%d", fn, (int)n_bad);
  return 0;
}

extern "C" int gvl_logits_process(void* logits, int64_t ld, int32_t logits_fp32, int64_t R,
                                  int64_t V, const int64_t* hist, int64_t hist_ld, int32_t n_hist,
                                  const int32_t* src, int64_t src_ld, int64_t t0,
                                  const int64_t* prompt, int64_t prompt_ld, int32_t P,
                                  int32_t rows_per_item, float rep_penalty, int32_t ngram,
                                  int32_t eos, int32_t ban_eos, const int32_t* bad, int32_t n_bad,
                                  const int32_t* flen, gvl_stream_t stream) {
  if (check_logits("gvl_logits_process", "n_hist", logits, ld, R, V, hist, hist_ld, n_hist, src,
                   src_ld, t0, prompt, prompt_ld, P, rows_per_item, rep_penalty, ngram, bad, n_bad))
    return -1;
  if (R == 0) return 0;
  if (rep_penalty == 1.f && ngram == 0 && !ban_eos && n_bad == 0) return 0;  // every control off
  LogitsP p{logits, ld, R, V, logits_fp32, hist, hist_ld, n_hist, src, src_ld, t0, prompt,
            prompt_ld, P, rows_per_item, rep_penalty, ngram, eos, ban_eos, bad, n_bad, flen};
  hipLaunchKernelGGL(logits_process_kernel, dim3((unsigned)R), dim3(LP_NT), 0,
                     gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK("gvl_logits_process");
  return 0;
}

extern "C" int gvl_logits_process_dev(void* logits, int64_t ld, int32_t logits_fp32, int64_t R,
                                      int64_t V, const int64_t* hist, int64_t hist_ld,
                                      const int32_t* step, int32_t hist_cap, const int32_t* src,
                                      int64_t src_ld, int64_t t0, const int64_t* prompt,
                                      int64_t prompt_ld, int32_t P, int32_t rows_per_item,
                                      float rep_penalty, int32_t ngram, int32_t eos,
                                      int32_t min_new, const int32_t* bad, int32_t n_bad,
                                      const int32_t* flen, gvl_stream_t stream) {
  GVL_REQUIRE(step != nullptr, "gvl_logits_process_dev: null step");
  if (check_logits("gvl_logits_process_dev", "hist_cap", logits, ld, R, V, hist, hist_ld, hist_cap,
                   src, src_ld, t0, prompt, prompt_ld, P, rows_per_item, rep_penalty, ngram, bad,
                   n_bad))
    return -1;
  if (R == 0) return 0;
  if (rep_penalty == 1.f && ngram == 0 && min_new <= 0 && n_bad == 0) return 0;  // every control off
  LogitsP p{logits, ld, R, V, logits_fp32, hist, hist_ld, 0, src, src_ld, t0, prompt,
            prompt_ld, P, rows_per_item, rep_penalty, ngram, eos, 0, bad, n_bad, flen};
  hipLaunchKernelGGL(logits_process_dev_kernel, dim3((unsigned)R), dim3(LP_NT), 0,
                     gvl::as_stream(stream), p, step, (int)hist_cap, (int)min_new);
  GVL_LAUNCH_CHECK("gvl_logits_process_dev");
  return 0;
}
