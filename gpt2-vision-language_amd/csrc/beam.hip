// One beam-search step (include/gvl.h gvl_beam_step) in two launches, both latency-bound.
//
// beam_rows_kernel: one 1024-thread workgroup per row r = b*K + j, the row (V <= 65536) in
// registers as contiguous 64-element chunks like sample_kernel.  A live row turns its logits
// into raw scores score_in + log_softmax (fp32, max subtracted) and takes its K best by K
// rounds of a block arg-max on key = raw * len_norm[step + 1] (ties: the lower token id);
// K <= 8, so K rounds of 64 compares per thread cost less than a radix select's four passes
// and keep the tie rule exact.  A finished row passes its one (eos) candidate on, an empty
// row none.  The K candidates of every row go to the caller's workspace.
//
// beam_merge_kernel: one 256-thread workgroup per item.  The K*K <= 64 candidates are ranked by
// counting, per candidate, those that beat it (greater key; equal key: lower parent slot, then
// lower token id) — ranks are distinct because (parent, token) pairs are.  Rank i < K fills
// output slot i; the slots past the last candidate are written empty.  Then the block gathers
// the parents' rows of the cache indirection table and appends each new row's own index.
#include "common.h"
#include "capi_util.h"
#include "../../include/gvl.h"

namespace {

constexpr int BM_NT = 1024;
constexpr int BM_E = 64;  // elements per thread: V <= 65536
constexpr int BM_MAXK = 8;
constexpr int MG_NT = 256;
constexpr uint32_t BM_NONE = 0xFFFFFFFFu;

struct BeamCand {
  float key, raw;
  int32_t tok, flen;  // tok < 0: no candidate
};

struct BeamP {
  const void* logits;
  int64_t ld, V;
  int f32, K, step, eos;
  const float* score_in;
  const int32_t* flen_in;
  const float* len_norm;
  BeamCand* cand;  // [rows][K]
  int64_t t0, src_ld;
  const int32_t* src_in;
  int64_t* tok_out;
  int32_t* parent_out;
  float* score_out;
  int32_t* flen_out;
  int32_t* src_out;
};

// (key, idx) a beats b: the greater key, then the lower index; BM_NONE (nothing yet) loses to
// every real index, whatever its key
GVL_DEV bool cand_beats(float ka, uint32_t ia, float kb, uint32_t ib) {
  if (ia == BM_NONE) return false;
  if (ib == BM_NONE) return true;
  return ka > kb || (ka == kb && ia < ib);
}

// The bodies of both pairs of kernels: `step` comes from the launch arguments (gvl_beam_step) or
// from device memory (gvl_beam_step_dev); p.step itself goes unused.
GVL_DEV void beam_rows_body(const BeamP& p, int step) {
  __shared__ float red[BM_NT / 64];
  __shared__ float s_key[BM_NT / 64];
  __shared__ float s_raw[BM_NT / 64];
  __shared__ uint32_t s_idx[BM_NT / 64];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  BeamCand* out = p.cand + row * p.K;
  const float sc = p.score_in[row];
  const int fl = p.flen_in[row];
  if (sc == -INFINITY || fl > 0) {  // (block-uniform) empty: nothing; finished: itself
    if (tid < p.K) {
      BeamCand c{-INFINITY, -INFINITY, -1, 0};
      if (tid == 0 && sc != -INFINITY) c = BeamCand{sc * p.len_norm[fl], sc, p.eos >= 0 ? p.eos : 0, fl};
      out[tid] = c;
    }
    return;
  }
  const int E = (int)((p.V + BM_NT - 1) / BM_NT);
  const int64_t i0 = (int64_t)tid * E;
  float x[BM_E];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < BM_E; ++j) {
    const int64_t i = i0 + j;
    float v = -INFINITY;
    if (j < E && i < p.V)
      v = p.f32 ? reinterpret_cast<const float*>(p.logits)[row * p.ld + i]
                : bf2f(reinterpret_cast<const bf16_t*>(p.logits)[row * p.ld + i]);
    x[j] = v;
    mx = fmaxf(mx, v);
  }
  mx = block_max<BM_NT>(mx, red);
  float z = 0.f;
#pragma unroll
  for (int j = 0; j < BM_E; ++j)
    z += (x[j] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((x[j] - mx) * 1.4426950408889634f);
  z = block_sum<BM_NT>(z, red);
  const float lz = logf(z);
  const float ln = p.len_norm[step + 1];
  // raw score of token i0 + j; NaN: not a candidate (past the row's end, or already selected)
#pragma unroll
  for (int j = 0; j < BM_E; ++j)
    x[j] = (j < E && i0 + j < p.V) ? sc + ((x[j] - mx) - lz) : __builtin_nanf("");

  const int lane = tid & 63, w = tid >> 6;
  for (int i = 0; i < p.K; ++i) {
    float bk = -INFINITY, br = -INFINITY;
    uint32_t bi = BM_NONE;
#pragma unroll
    for (int j = 0; j < BM_E; ++j) {
      const float k = x[j] * ln;
      if (x[j] == x[j] && (bi == BM_NONE || k > bk)) {  // ascending j: a tie keeps the lower id
        bk = k;
        br = x[j];
        bi = (uint32_t)(i0 + j);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float k2 = __shfl_xor(bk, o, 64), r2 = __shfl_xor(br, o, 64);
      const uint32_t i2 = __shfl_xor(bi, o, 64);
      if (cand_beats(k2, i2, bk, bi)) {
        bk = k2;
        br = r2;
        bi = i2;
      }
    }
    __syncthreads();  // (the previous round's reads of s_* are done)
    if (lane == 0) {
      s_key[w] = bk;
      s_raw[w] = br;
      s_idx[w] = bi;
    }
    __syncthreads();
    bk = s_key[0];
    br = s_raw[0];
    bi = s_idx[0];
#pragma unroll
    for (int g = 1; g < BM_NT / 64; ++g)
      if (cand_beats(s_key[g], s_idx[g], bk, bi)) {
        bk = s_key[g];
        br = s_raw[g];
        bi = s_idx[g];
      }
#pragma unroll
    for (int j = 0; j < BM_E; ++j)
      if (j < E && bi == (uint32_t)(i0 + j)) x[j] = __builtin_nanf("");
    if (tid == 0) {
      BeamCand c{bk, br, (int32_t)bi, 0};
      if (bi == BM_NONE) c = BeamCand{-INFINITY, -INFINITY, -1, 0};  // (V >= K: not reached)
      else if ((int32_t)bi == p.eos) c.flen = step + 1;
      out[i] = c;
    }
  }
}

GVL_DEV void beam_merge_body(const BeamP& p, int step) {
  __shared__ BeamCand c[BM_MAXK * BM_MAXK];
  __shared__ int par[BM_MAXK];
  __shared__ int nvalid;
  const int tid = threadIdx.x, K = p.K, KK = p.K * p.K;
  const int64_t r0 = (int64_t)blockIdx.x * K;
  if (tid < KK) c[tid] = p.cand[r0 * K + tid];  // candidate tid: parent slot tid / K
  if (tid < K) par[tid] = tid;
  if (tid == 0) nvalid = 0;
  __syncthreads();
  if (tid < KK && c[tid].tok >= 0) {
    atomicAdd(&nvalid, 1);
    const BeamCand me = c[tid];
    const int pm = tid / K;
    int rank = 0;
    for (int o = 0; o < KK; ++o) {
      const BeamCand ot = c[o];
      const int po = o / K;
      if (o != tid && ot.tok >= 0 &&
          (ot.key > me.key || (ot.key == me.key && (po < pm || (po == pm && ot.tok < me.tok)))))
        ++rank;
    }
    if (rank < K) {
      p.tok_out[r0 + rank] = me.tok;
      p.parent_out[r0 + rank] = pm;
      p.score_out[r0 + rank] = me.raw;
      p.flen_out[r0 + rank] = me.flen;
      par[rank] = pm;
    }
  }
  __syncthreads();
  if (tid < K && tid >= nvalid) {  // fewer than K candidates: the remaining slots are empty
    p.tok_out[r0 + tid] = p.eos >= 0 ? p.eos : 0;
    p.parent_out[r0 + tid] = tid;
    p.score_out[r0 + tid] = -INFINITY;
    p.flen_out[r0 + tid] = 0;
  }
  const int64_t T = p.t0 + step;  // positions already in the cache
  for (int64_t idx = tid; idx < (int64_t)K * T; idx += MG_NT) {
    const int i = (int)(idx / T);
    const int64_t t = idx - (int64_t)i * T;
    p.src_out[(r0 + i) * p.src_ld + t] = p.src_in[(r0 + par[i]) * p.src_ld + t];
  }
  if (tid < K) p.src_out[(r0 + tid) * p.src_ld + T] = (int32_t)(r0 + tid);
}

__global__ __launch_bounds__(BM_NT) void beam_rows_kernel(BeamP p) { beam_rows_body(p, p.step); }
__global__ __launch_bounds__(MG_NT) void beam_merge_kernel(BeamP p) { beam_merge_body(p, p.step); }

// gvl_beam_step_dev: (block-uniform) a step outside [0, max_steps) writes nothing.
__global__ __launch_bounds__(BM_NT) void beam_rows_dev_kernel(BeamP p, const int32_t* step,
                                                              int max_steps) {
  const int st = *step;
  if (st < 0 || st >= max_steps) return;
  beam_rows_body(p, st);
}
__global__ __launch_bounds__(MG_NT) void beam_merge_dev_kernel(BeamP p, const int32_t* step,
                                                               int max_steps) {
  const int st = *step;
  if (st < 0 || st >= max_steps) return;
  beam_merge_body(p, st);
}

}  // namespace

extern "C" int64_t gvl_beam_step_workspace_size(int64_t B, int32_t K) {
  if (B <= 0 || K <= 0) return 0;
  return B * K * K * (int64_t)sizeof(BeamCand);
}

// What both entry points require alike; `step` is the furthest step the launch can take
// (gvl_beam_step_dev: max_steps - 1).
static int check_beam(const char* fn, const void* logits, int64_t ld, int64_t B, int32_t K,
                      int64_t V, const float* score_in, const int32_t* flen_in,
                      const float* len_norm, int32_t step, int32_t eos, int64_t t0,
                      const int32_t* src_in, int64_t src_ld, int64_t* tok_out, int32_t* parent_out,
                      float* score_out, int32_t* flen_out, int32_t* src_out, void* workspace) {
  GVL_REQUIRE(logits && score_in && flen_in && len_norm && src_in && tok_out && parent_out &&
                  score_out && flen_out && src_out && workspace,
              "%s: null buffer", fn);
  GVL_REQUIRE(K >= 1 && K <= BM_MAXK, "%s: K=%d out of range (1..%d)", fn, (int)K, BM_MAXK);
  GVL_REQUIRE(V >= K && V <= (int64_t)BM_NT * BM_E, "%s: V=%lld out of range (K=%d..%d)", fn,
              (long long)V, (int)K, BM_NT * BM_E);
  GVL_REQUIRE(ld >= V, "%s: ld=%lld < V=%lld", fn, (long long)ld, (long long)V);
  GVL_REQUIRE(B >= 0 && B * K <= 0x7fffffff / BM_MAXK, "%s: B=%lld out of range", fn, (long long)B);
  GVL_REQUIRE(eos >= -1 && eos < V, "%s: eos=%d outside the vocabulary", fn, (int)eos);
  GVL_REQUIRE(step >= 0 && t0 >= 0 && t0 + step < src_ld,
              "%s: position t0 + step = %lld outside the src table (src_ld=%lld)", fn,
              (long long)(t0 + step), (long long)src_ld);
  GVL_REQUIRE(src_in != src_out, "%s: src_in and src_out must be distinct tables", fn);
  GVL_REQUIRE(gvl::aligned8(workspace), "%s: workspace must be 8-byte aligned", fn);
  return 0;
}

extern "C" int gvl_beam_step(const void* logits, int64_t ld, int32_t logits_fp32, int64_t B,
                             int32_t K, int64_t V, const float* score_in, const int32_t* flen_in,
                             const float* len_norm, int32_t step, int32_t eos, int64_t t0,
                             const int32_t* src_in, int64_t src_ld, int64_t* tok_out,
                             int32_t* parent_out, float* score_out, int32_t* flen_out,
                             int32_t* src_out, void* workspace, gvl_stream_t stream) {
  if (check_beam("gvl_beam_step", logits, ld, B, K, V, score_in, flen_in, len_norm, step, eos, t0,
                 src_in, src_ld, tok_out, parent_out, score_out, flen_out, src_out, workspace))
    return -1;
  if (B == 0) return 0;
  BeamP p{logits, ld, V, logits_fp32, K, step, eos, score_in, flen_in, len_norm,
          static_cast<BeamCand*>(workspace), t0, src_ld, src_in, tok_out, parent_out, score_out,
          flen_out, src_out};
  hipLaunchKernelGGL(beam_rows_kernel, dim3((unsigned)(B * K)), dim3(BM_NT), 0,
                     gvl::as_stream(stream), p);
  GVL_LAUNCH_CHECK("gvl_beam_step");
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)B), dim3(MG_NT), 0, gvl::as_stream(stream),
                     p);
  GVL_LAUNCH_CHECK("gvl_beam_step");
  return 0;
}

extern "C" int gvl_beam_step_dev(const void* logits, int64_t ld, int32_t logits_fp32, int64_t B,
                                 int32_t K, int64_t V, const float* score_in,
                                 const int32_t* flen_in, const float* len_norm,
                                 const int32_t* step, int32_t max_steps, int32_t eos, int64_t t0,
                                 const int32_t* src_in, int64_t src_ld, int64_t* tok_out,
                                 int32_t* parent_out, float* score_out, int32_t* flen_out,
                                 int32_t* src_out, void* workspace, gvl_stream_t stream) {
  GVL_REQUIRE(step != nullptr, "gvl_beam_step_dev: null step");
  GVL_REQUIRE(max_steps >= 1, "gvl_beam_step_dev: max_steps=%d must be at least 1", (int)max_steps);
  if (check_beam("gvl_beam_step_dev", logits, ld, B, K, V, score_in, flen_in, len_norm,
                 max_steps - 1, eos, t0, src_in, src_ld, tok_out, parent_out, score_out, flen_out,
                 src_out, workspace))
    return -1;
  if (B == 0) return 0;
  BeamP p{logits, ld, V, logits_fp32, K, 0, eos, score_in, flen_in, len_norm,
          static_cast<BeamCand*>(workspace), t0, src_ld, src_in, tok_out, parent_out, score_out,
          flen_out, src_out};
  hipLaunchKernelGGL(beam_rows_dev_kernel, dim3((unsigned)(B * K)), dim3(BM_NT), 0,
                     gvl::as_stream(stream), p, step, (int)max_steps);
  GVL_LAUNCH_CHECK("gvl_beam_step_dev");
  hipLaunchKernelGGL(beam_merge_dev_kernel, dim3((unsigned)B), dim3(MG_NT), 0,
                     gvl::as_stream(stream), p, step, (int)max_steps);
  GVL_LAUNCH_CHECK("gvl_beam_step_dev");
  return 0;
}
