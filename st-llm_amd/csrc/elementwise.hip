// HBM-bound glue kernels: row gather (token-block assembly / masking / embedding lookup),
// temporal mean, ViT CLS rows, MVM cosine loss rows.  All fp32, float4-vectorised, coalesced.
// Below them: the KV-cache append / re-order copies, and token selection on a logits row held in the LDS (stllm_select_tokens, stllm_beam_candidates).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src_a, int64_t ld_a,
                                                          const float* __restrict__ src_b, int64_t ld_b,
                                                          const int32_t* __restrict__ idx_a,
                                                          const float* __restrict__ add, int64_t ld_add,
                                                          const int32_t* __restrict__ idx_add,
                                                          float* __restrict__ dst, int64_t ld_dst, int n_rows, int D,
                                                          float scale) {
  const int row = blockIdx.x;
  if (row >= n_rows) return;
  const int ia = idx_a[row];
  const float4* s = (ia >= 0) ? reinterpret_cast<const float4*>(src_a + (int64_t)ia * ld_a)
                              : reinterpret_cast<const float4*>(src_b + (int64_t)(-ia - 1) * ld_b);
  const float4* a = add ? reinterpret_cast<const float4*>(add + (int64_t)idx_add[row] * ld_add) : nullptr;
  float4* d = reinterpret_cast<float4*>(dst + (int64_t)row * ld_dst);
  for (int c = threadIdx.x; c < (D >> 2); c += blockDim.x) {
    float4 v = s[c];
    if (a) { const float4 w = a[c]; v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w; }
    if (scale != 1.0f) { v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale; }
    d[c] = v;
  }
}

__global__ __launch_bounds__(256) void mean_t_kernel(const float* __restrict__ x, float* __restrict__ out, int T,
                                                     int64_t J4) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (j >= J4) return;
  const float4* xb = reinterpret_cast<const float4*>(x) + (int64_t)b * T * J4 + j;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = 0; t < T; ++t) {
    const float4 v = xb[(int64_t)t * J4];
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  const float inv = 1.0f / (float)T;
  acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
  reinterpret_cast<float4*>(out)[(int64_t)b * J4 + j] = acc;
}

__global__ __launch_bounds__(256) void cls_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                                       float* __restrict__ x, int64_t ldx, int D) {
  const int n = blockIdx.x;
  float* d = x + (int64_t)n * 257 * ldx;
  for (int c = threadIdx.x; c < D; c += blockDim.x) d[c] = cls[c] + pos[c];
}

__global__ __launch_bounds__(256) void cosine_rows_kernel(const float* __restrict__ a, int64_t lda,
                                                          const int32_t* __restrict__ idx_a,
                                                          const float* __restrict__ b, int64_t ldb,
                                                          const int32_t* __restrict__ idx_b, float* __restrict__ out,
                                                          int n_rows, int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const float4* ar = reinterpret_cast<const float4*>(a + (int64_t)(idx_a ? idx_a[row] : row) * lda);
  const float4* br = reinterpret_cast<const float4*>(b + (int64_t)(idx_b ? idx_b[row] : row) * ldb);
  float ab = 0.f, aa = 0.f, bb = 0.f;
  for (int c = lane; c < (D >> 2); c += 64) {
    const float4 u = ar[c], v = br[c];
    ab += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
    aa += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
    bb += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ab = wave_sum(ab); aa = wave_sum(aa); bb = wave_sum(bb);
  if (lane == 0) out[row] = 2.0f - 2.0f * ab / (sqrtf(aa) * sqrtf(bb));
}

// per-row cross-entropy: loss[i] = logsumexp(logits[i,:]) - logits[i,label[i]]; label < 0 -> 0
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, int64_t ldl,
                                                      const int32_t* __restrict__ labels, float* __restrict__ loss,
                                                      int V) {
  __shared__ float red[4];
  const int row = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lab = labels[row];
  if (lab < 0) { if (threadIdx.x == 0) loss[row] = 0.0f; return; }
  const float* x = logits + (int64_t)row * ldl;
  float mx = -3.0e38f;
  for (int c = threadIdx.x; c < V; c += 256) mx = fmaxf(mx, x[c]);
  mx = wave_max(mx);
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.0f;
  for (int c = threadIdx.x; c < V; c += 256) s += expf(x[c] - mx);
  s = wave_sum(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[row] = logf(red[0] + red[1] + red[2] + red[3]) + mx - x[lab];
}

// fp32 -> compute dtype rows (A operand of a GEMM whose input lives in the fp32 residual stream)
template <typename T>
__global__ __launch_bounds__(256) void cast_rows_kernel(const float* __restrict__ x, int64_t ldx, void* __restrict__ out,
                                                        int64_t ldo, int D) {
  const int row = blockIdx.x;
  const float4* xr = reinterpret_cast<const float4*>(x + (int64_t)row * ldx);
  for (int c = threadIdx.x; c < (D >> 2); c += blockDim.x) {
    const float4 v = xr[c];
    if constexpr (Elem<T>::kIsF32) {
      reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + (int64_t)row * ldo)[c] = v;
    } else {
      uint2 pk;
      pk.x = Elem<T>::pack2(v.x, v.y);
      pk.y = Elem<T>::pack2(v.z, v.w);
      reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out) + (int64_t)row * ldo)[c] = pk;
    }
  }
}

// ragged KV-cache append: the [k | v] (or [q | k | v]) bytes of dense row b -> the cache row of batch entry b at position pos[b]; 16 bytes per lane.
// A position outside [0, max_len) marks a free slot of the batch: nothing is written for it.
__global__ __launch_bounds__(256) void kv_append_rows_kernel(const char* __restrict__ src, int64_t src_stride, char* __restrict__ cache,
                                                             int64_t batch_stride, int64_t row_stride, const int32_t* __restrict__ pos,
                                                             int max_len, int col0_bytes, int n16) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  const int ps = pos[b];
  if (c >= n16 || ps < 0 || ps >= max_len) return;
  const uint4 v = reinterpret_cast<const uint4*>(src + (int64_t)b * src_stride + col0_bytes)[c];
  reinterpret_cast<uint4*>(cache + (int64_t)b * batch_stride + (int64_t)ps * row_stride + col0_bytes)[c] = v;
}

// ragged KV-cache append of token BLOCKS (stllm_kv_append_spans): the [k | v] bytes of dense row b * S + i -> the cache row of batch entry b at position
// pos0[b] + i, for i < min(n[b], S); 16 bytes per lane, blockIdx.y = b * S + i.  Pad rows (i >= n[b]) and positions outside [0, max_len) write nothing.
__global__ __launch_bounds__(256) void kv_append_spans_kernel(const char* __restrict__ src, int64_t src_stride, char* __restrict__ cache,
                                                              int64_t batch_stride, int64_t row_stride, const int32_t* __restrict__ pos0,
                                                              const int32_t* __restrict__ n, int S, int max_len, int col0_bytes, int n16) {
  const int r = blockIdx.y, b = r / S, i = r - b * S, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n16 || i >= n[b]) return;
  const int64_t ps = (int64_t)pos0[b] + i;
  if (ps < 0 || ps >= max_len) return;
  const uint4 v = reinterpret_cast<const uint4*>(src + (int64_t)r * src_stride + col0_bytes)[c];
  reinterpret_cast<uint4*>(cache + (int64_t)b * batch_stride + ps * row_stride + col0_bytes)[c] = v;
}

// kv_append_spans_kernel for a PACKED source (stllm_kv_append_segments): the [k | v] bytes of packed row row0[r] + i -> cache row slot[r] at position
// pos0[r] + i, for i < n[r]; blockIdx.z = segment r, blockIdx.y = i.  A segment whose slot is outside [0, n_slots) or whose packed rows are outside [0, T)
// writes nothing (the table guard of stllm_attention_segments), as do positions outside [0, max_len).
__global__ __launch_bounds__(256) void kv_append_segments_kernel(const char* __restrict__ src, int64_t src_stride, char* __restrict__ cache,
                                                                 int64_t batch_stride, int64_t row_stride, const int32_t* __restrict__ slot,
                                                                 const int32_t* __restrict__ row0, const int32_t* __restrict__ pos0,
                                                                 const int32_t* __restrict__ n, int T, int n_slots, int max_len, int col0_bytes, int n16) {
  const int r = blockIdx.z, i = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  const int nr = n[r], sl = slot[r], r0 = row0[r];
  if (c >= n16 || i >= nr) return;
  if (sl < 0 || sl >= n_slots || r0 < 0 || (int64_t)r0 + nr > T) return;
  const int64_t ps = (int64_t)pos0[r] + i;
  if (ps < 0 || ps >= max_len) return;
  const uint4 v = reinterpret_cast<const uint4*>(src + (int64_t)(r0 + i) * src_stride + col0_bytes)[c];
  reinterpret_cast<uint4*>(cache + (int64_t)sl * batch_stride + ps * row_stride + col0_bytes)[c] = v;
}

// in-place re-order of the cache rows of beam groups (stllm_kv_reorder_rows): group g = blockIdx.y is rows [g * nb, (g + 1) * nb), row r takes the [k | v]
// bytes of row src[r] at the positions [max(lo[g], 0), min(hi[g], capacity)).  One thread owns one 16-byte cell (position, column piece) of the group:
// it loads the cell from all nb rows, then stores the rows whose source differs — no other thread touches that cell in any row of the group, so a cycle
// needs no scratch and no barrier.  cell[] and l[] are indexed with compile-time indices only (unrolled to kReorderMaxBeams, predicated on j < nb: the
// table is uniform over the block, so the predicates are scalar branches) and stay in registers.  `cache` is deliberately not __restrict__: the stores
// alias the loads, and every load stays in front of every store.  A src entry outside its own group is the identity.
constexpr int kReorderMaxBeams = 16;

// the per-row steps as compile-time recursions over the row index: every cell[] / l[] index is a constant in the source, whatever the unroller decides
template <int J>
__device__ __forceinline__ void reorder_table(int (&l)[kReorderMaxBeams], bool& any, const int32_t* src, int row0, int nb) {
  if constexpr (J < kReorderMaxBeams) {
    l[J] = J;
    if (J < nb) {
      const int s = src[row0 + J] - row0;   // local to the group; outside it: the identity
      if (s >= 0 && s < nb) l[J] = s;
      any = any || l[J] != J;
    }
    reorder_table<J + 1>(l, any, src, row0, nb);
  }
}

template <int J>
__device__ __forceinline__ void reorder_load(uint4 (&cell)[kReorderMaxBeams], const uint4* p, int64_t rs16, int nb) {
  if constexpr (J < kReorderMaxBeams) {
    if (J < nb) cell[J] = p[J * rs16];
    reorder_load<J + 1>(cell, p, rs16, nb);
  }
}

// cell[l] as a chain of selects on VALUES (l is uniform: scalar compares): branches that each store cell[I] are merged by the optimiser into one store
// of cell[l] with a run-time index, which puts the array into scratch
template <int I>
__device__ __forceinline__ uint4 reorder_pick(const uint4 (&cell)[kReorderMaxBeams], int l, int nb, uint4 v) {
  if constexpr (I < kReorderMaxBeams) {
    if (I < nb) {
      const bool hit = l == I;
      v.x = hit ? cell[I].x : v.x; v.y = hit ? cell[I].y : v.y; v.z = hit ? cell[I].z : v.z; v.w = hit ? cell[I].w : v.w;
    }
    return reorder_pick<I + 1>(cell, l, nb, v);
  } else {
    return v;
  }
}

template <int J>
__device__ __forceinline__ void reorder_store(const uint4 (&cell)[kReorderMaxBeams], const int (&l)[kReorderMaxBeams], uint4* p, int64_t rs16, int nb) {
  if constexpr (J < kReorderMaxBeams) {
    if (J < nb && l[J] != J) p[J * rs16] = reorder_pick<0>(cell, l[J], nb, cell[J]);
    reorder_store<J + 1>(cell, l, p, rs16, nb);
  }
}

__global__ __launch_bounds__(256) void kv_reorder_rows_kernel(char* cache, int64_t batch_stride, int64_t row_stride, const int32_t* __restrict__ src,
                                                              const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int nb, int capacity,
                                                              int col0_bytes, int n16) {
  const int g = blockIdx.y;
  const int p0 = max(lo[g], 0), p1 = min(hi[g], capacity);
  if (p1 <= p0) return;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ps = p0 + c / n16;
  if (ps >= p1) return;
  const int col = (int)(c % n16);
  int l[kReorderMaxBeams];                        // source of row j, local to the group; j: nothing to do
  bool any = false;
  reorder_table<0>(l, any, src, g * nb, nb);
  if (!any) return;
  uint4* cellp = reinterpret_cast<uint4*>(cache + (int64_t)g * nb * batch_stride + ps * row_stride + col0_bytes) + col;
  const int64_t rs16 = batch_stride / 16;         // between the rows of the group, in cells
  uint4 cell[kReorderMaxBeams];
  reorder_load<0>(cell, cellp, rs16, nb);
  reorder_store<0>(cell, l, cellp, rs16, nb);
}

// ---- token selection: stllm_select_tokens / stllm_beam_candidates (include/stllm_hip.h) --------------------------------------------------------------
// One workgroup per row; the row lives in the LDS as fp32 from the staging on (V <= ~40 k floats), every later pass reads the LDS.  Reductions: a
// per-thread partial in index order, the xor butterfly inside a wave, the four wave results combined in a fixed order — no atomics, so a launch is
// bit-reproducible.  The four-entry exchange buffers are double-buffered by `ph`: one barrier per reduction.
constexpr int kSelThreads = 256;
constexpr int kSelLdsBytes = 160 * 1024 - 4096;   // dynamic LDS a row may take: the CU's 160 KiB less the static scratch below
constexpr float kSelNoIndex = 3.0e38f;            // "no candidate yet" index (indices travel as floats: V < 2^24)

struct SelRed { float v[2][4]; float i[2][4]; };

__device__ __forceinline__ float sel_block_sum(float v, SelRed* red, int& ph) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red->v[ph][threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (red->v[ph][0] + red->v[ph][1]) + (red->v[ph][2] + red->v[ph][3]);
  ph ^= 1;
  return r;
}

// (value, index) of the best entry of the block under (value descending, index ascending); every thread receives it
__device__ __forceinline__ void sel_block_best(float& v, float& i, SelRed* red, int& ph) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64), oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  if ((threadIdx.x & 63) == 0) { red->v[ph][threadIdx.x >> 6] = v; red->i[ph][threadIdx.x >> 6] = i; }
  __syncthreads();
  v = red->v[ph][0]; i = red->i[ph][0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float ov = red->v[ph][w], oi = red->i[ph][w];
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  ph ^= 1;
}

// repetition penalty on the staged row: every id's new value is computed from the ORIGINAL score into pv[j] before any score is rewritten, so a
// repeated id writes the same value again (once per distinct id).  Ids outside [0, V) are skipped.  Ends with the row visible to every thread.
__device__ __forceinline__ void sel_penalise(float* s, float* pv, const int32_t* prev, int n_prev, int V, float pen) {
  for (int j = threadIdx.x; j < n_prev; j += kSelThreads) {
    const int id = prev[j];
    if ((unsigned)id < (unsigned)V) { const float x = s[id]; pv[j] = x < 0.0f ? x * pen : __fdiv_rn(x, pen); }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_prev; j += kSelThreads) {
    const int id = prev[j];
    if ((unsigned)id < (unsigned)V) s[id] = pv[j];
  }
  __syncthreads();
}

// One kernel body for stllm_select_tokens (SLOTS = false: workgroup = row r of every table, one step index for the launch) and stllm_select_slots
// (SLOTS = true: workgroup = slot, which reads logits row src[slot] behind its own history, step count and EOS suppression, and whose thread 0 appends
// the token and updates the slot's state row at the end).  Everything between the staging and the token is the same code: steps 1 - 3 of the header.
template <bool SLOTS> struct SelArgs { typedef stllm_select_args type; };
template <> struct SelArgs<true> { typedef stllm_select_slots_args type; };

// stllm_select_slots, thread 0: the token is appended at ids[c]; `live` drops on EOS, at the budget, or when the history now ends in a stop sequence (its
// last id is this step's token, the others are ids[c + 1 - n ..])
__device__ __forceinline__ void sel_slot_update(const stllm_select_slots_args& a, int32_t* st, int32_t* hist, int c, int max_new, int tok) {
  int live = (tok == a.eos_id || c + 1 >= max_new) ? 0 : 1;
  for (int j = 0; live && j < a.n_stop; ++j) {
    const int n = a.stop_len[j];
    if (n <= 0 || n > c + 1 || n > a.ld_stop) continue;
    const int32_t* sq = a.stops + (int64_t)j * a.ld_stop;
    bool hit = sq[n - 1] == tok;
    for (int i = 0; hit && i < n - 1; ++i) hit = hist[c + 1 - n + i] == sq[i];
    if (hit) live = 0;
  }
  hist[c] = tok;
  st[1] = c + 1;
  st[3] = tok;
  st[0] = live;
}

template <bool SLOTS>
__global__ __launch_bounds__(kSelThreads) void select_kernel(const typename SelArgs<SLOTS>::type a) {
  extern __shared__ float smem[];                 // [V] scores, then [n_prev] penalised values
  __shared__ SelRed red;
  __shared__ float csum[kSelThreads];             // per-chunk kept sums, then their inclusive prefix
  __shared__ int clast[kSelThreads];              // last kept id of a chunk, -1: none
  __shared__ float gbase[kSelThreads / 16];
  int row = blockIdx.x;                           // of u and aux (the slot), and of every other table of stllm_select_tokens
  const int tid = threadIdx.x, V = a.V;
  // what differs between the two entry points, set once: where the token goes, the logits row, the history and the EOS suppression
  int32_t* out = nullptr;
  int32_t *st = nullptr, *hist = nullptr;
  int hist_n = 0, max_new = 0;
  const float* x;
  const int32_t* prev;
  int n_prev;
  bool suppress_eos;
  if constexpr (SLOTS) {
    const int r = a.src[row];
    if (r < 0 || r >= a.rows) return;             // not served in this step (uniform over the block): nothing else is read
    st = a.state + (int64_t)row * 4;              // (live, n_gen, max_new, pending): read here by every thread, written by thread 0 behind the barriers
    if (st[0] == 0) {
      if (tid == 0) st[3] = a.pad_id;
      return;
    }
    const int n_gen = st[1];
    max_new = st[2];
    hist_n = min(max(n_gen, 0), (int)a.ld_ids - 1);
    hist = a.ids + (int64_t)row * a.ld_ids;
    x = a.logits + (int64_t)r * a.ldl;
    prev = hist; n_prev = hist_n;
    suppress_eos = a.eos_id >= 0 && n_gen < a.min_length;
  } else {
    out = a.out + (int64_t)row * a.out_stride;
    if (a.unfinished && a.unfinished[row] == 0) {   // a finished row emits pad (uniform over the block)
      if (tid == 0) *out = a.pad_id;
      return;
    }
    x = a.logits + (int64_t)row * a.ldl;
    prev = a.prev + (int64_t)row * a.ld_prev; n_prev = a.n_prev;
    suppress_eos = a.suppress_eos;
  }
  float* s = smem;
  for (int c = tid; c < V; c += kSelThreads) s[c] = x[c];
  __syncthreads();
  if (a.penalty != 1.0f && n_prev > 0) sel_penalise(s, s + V, prev, n_prev, V, a.penalty);
  if (suppress_eos && tid == 0 && (unsigned)a.eos_id < (unsigned)V) s[a.eos_id] = -INFINITY;
  __syncthreads();
  // from here to the chunked walk a thread touches only the columns c = tid (mod 256): no barrier is needed between those passes
  const bool sample = a.sample != 0;
  const bool warm = sample && a.temperature != 1.0f;
  int ph = 0;
  float bv = -INFINITY, bi = kSelNoIndex;
  for (int c = tid; c < V; c += kSelThreads) {
    float v = s[c];
    if (warm) { v = __fdiv_rn(v, a.temperature); s[c] = v; }
    if (v > bv) { bv = v; bi = (float)c; }
  }
  sel_block_best(bv, bi, &red, ph);
  const float mx = bv;
  const int amax = bi < (float)V ? (int)bi : 0;
  if (!sample) {
    if (a.aux) {
      float z = 0.0f;
      for (int c = tid; c < V; c += kSelThreads) z += expf(s[c] - mx);
      z = sel_block_sum(z, &red, ph);
      if (tid == 0) { float* ax = a.aux + (int64_t)row * 4; ax[0] = mx; ax[1] = logf(z); ax[2] = 0.0f; ax[3] = 1.0f; }
    }
    if (tid == 0) {
      if constexpr (SLOTS) {
        sel_slot_update(a, st, hist, hist_n, max_new, amax);
      } else {
        *out = amax;
        if (a.unfinished && amax == a.eos_id) a.unfinished[row] = 0;
      }
    }
    return;
  }
  float z = 0.0f;
  for (int c = tid; c < V; c += kSelThreads) { const float e = expf(s[c] - mx); s[c] = e; z += e; }
  const float Z = sel_block_sum(z, &red, ph);
  // threshold = the smallest e-value t with sum_{e_j <= t} e_j > (1 - top_p) Z, found by bisection on the bit pattern (monotone for floats >= 0; the
  // masked sum runs in the same order every pass, so it is monotone in the mask).  exp(0) = 1 is the largest value there is.
  const uint32_t one = 0x3f800000u;
  uint32_t tb;
  if (a.top_p >= 1.0f) {
    tb = 1u;                                      // every e > 0
  } else {
    const float thr = (1.0f - a.top_p) * Z;
    if (!(Z > thr)) {
      tb = one + 1u;                              // nothing passes: the argmax alone (min_tokens_to_keep)
    } else {
      uint32_t lo = 0u, hi = one;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        float p = 0.0f;
#pragma unroll 8
        for (int c = tid; c < V; c += kSelThreads) { const float e = s[c]; p += __builtin_bit_cast(uint32_t, e) <= mid ? e : 0.0f; }   // (8 LDS reads in flight; the adds keep their order)
        p = sel_block_sum(p, &red, ph);
        if (p > thr) hi = mid; else lo = mid + 1u;
      }
      tb = lo;
    }
  }
  __syncthreads();                                // the walk owns contiguous chunks: other threads' e-values
  const int chunk = (V + kSelThreads - 1) / kSelThreads;
  const int c0 = min(V, tid * chunk), c1 = min(V, c0 + chunk);
  float cs = 0.0f;
  int last = -1;
  for (int c = c0; c < c1; ++c) {
    const float e = s[c];
    if (__builtin_bit_cast(uint32_t, e) >= tb || c == amax) { cs += e; last = c; }
  }
  csum[tid] = cs; clast[tid] = last;
  __syncthreads();
  if (tid != 0) return;
  // inclusive prefix of the chunk sums on two levels (16 x 16): no chain is longer than 32 adds
  float G = 0.0f;
  int lastk = amax;
  for (int g = 0; g < kSelThreads; g += 16) {
    float gs = 0.0f, run = G;
    gbase[g >> 4] = G;
    for (int t = g; t < g + 16; ++t) {
      const float c = csum[t];
      gs += c; run += c; csum[t] = run;
      if (clast[t] >= 0) lastk = clast[t];
    }
    G += gs;
  }
  const float Zk = G, target = a.u[row] * Zk;
  int tok = lastk;                                // rounding ran past the end: the last kept id
  for (int t = 0; t < kSelThreads; ++t) {
    if (clast[t] < 0 || !(csum[t] > target)) continue;
    float run = (t & 15) ? csum[t - 1] : gbase[t >> 4];
    tok = clast[t];
    const int d0 = min(V, t * chunk), d1 = min(V, d0 + chunk);
    for (int c = d0; c < d1; ++c) {
      const float e = s[c];
      if (__builtin_bit_cast(uint32_t, e) >= tb || c == amax) {
        run += e;
        if (run > target) { tok = c; break; }
      }
    }
    break;
  }
  if constexpr (SLOTS) {
    sel_slot_update(a, st, hist, hist_n, max_new, tok);
  } else {
    *out = tok;
    if (a.unfinished && tok == a.eos_id) a.unfinished[row] = 0;
  }
  if (a.aux) {
    float* ax = a.aux + (int64_t)row * 4;
    ax[0] = mx; ax[1] = logf(Z); ax[2] = __builtin_bit_cast(float, tb); ax[3] = __fdiv_rn(Zk, Z);
  }
}

// One kernel body for stllm_beam_candidates (ROWS = false: workgroup = row r of every table, one n_prev and one EOS suppression for the launch) and
// stllm_beam_candidates_rows (ROWS = true: workgroup = candidate row, which reads logits row src[row] behind its own history length and EOS suppression).
// What differs is set once at the top; everything behind it is the same code.
template <bool ROWS> struct BeamArgs { typedef stllm_beam_args type; };
template <> struct BeamArgs<true> { typedef stllm_beam_rows_args type; };

template <bool ROWS>
__global__ __launch_bounds__(kSelThreads) void beam_kernel(const typename BeamArgs<ROWS>::type a) {
  extern __shared__ float smem[];                 // [V] scores, then [n_prev] penalised values
  __shared__ SelRed red;
  const int row = blockIdx.x, tid = threadIdx.x, V = a.V;
  float* s = smem;
  const float* x;
  int n_prev;
  bool suppress_eos;
  if constexpr (ROWS) {
    const int r = a.src[row];
    if (r < 0 || r >= a.n_logits_rows) return;    // not served in this step (uniform over the block): nothing else is read
    const int n = a.n_prev[row];
    x = a.logits + (int64_t)r * a.ldl;
    n_prev = min(max(n, 0), (int)a.ld_prev);
    suppress_eos = a.eos_id >= 0 && n < a.min_length;
  } else {
    x = a.logits + (int64_t)row * a.ldl;
    n_prev = a.n_prev;
    suppress_eos = a.suppress_eos;
  }
  int ph = 0;
  float bv = -INFINITY, bi = kSelNoIndex;
  for (int c = tid; c < V; c += kSelThreads) {
    const float v = x[c];
    s[c] = v;
    if (v > bv) { bv = v; bi = (float)c; }
  }
  sel_block_best(bv, bi, &red, ph);
  const float mx = bv;
  float z = 0.0f;
  for (int c = tid; c < V; c += kSelThreads) z += expf(s[c] - mx);
  const float lse = logf(sel_block_sum(z, &red, ph));
  for (int c = tid; c < V; c += kSelThreads) s[c] = (s[c] - mx) - lse;   // log_softmax
  __syncthreads();
  if (a.penalty != 1.0f && n_prev > 0) sel_penalise(s, s + V, a.prev + (int64_t)row * a.ld_prev, n_prev, V, a.penalty);
  if (suppress_eos && tid == 0 && (unsigned)a.eos_id < (unsigned)V) s[a.eos_id] = -INFINITY;
  __syncthreads();
  const float bs = a.beam_score[row];
  for (int c = tid; c < V; c += kSelThreads) s[c] += bs;
  // k rounds of "the best entry strictly behind the previous pick" in the order (score descending, token ascending): nothing is rewritten, so
  // tied scores (-inf, or everything behind a -1e9 beam score) come out once each, in token order
  float lv = INFINITY, li = -1.0f;
  for (int r = 0; r < a.k; ++r) {
    bv = -INFINITY; bi = kSelNoIndex;
#pragma unroll 8
    for (int c = tid; c < V; c += kSelThreads) {
      const float v = s[c], fc = (float)c;
      if ((v < lv || (v == lv && fc > li)) && (v > bv || bi == kSelNoIndex)) { bv = v; bi = fc; }
    }
    sel_block_best(bv, bi, &red, ph);
    if (tid == 0) {
      a.cand_score[(int64_t)row * a.k + r] = bv;
      a.cand_token[(int64_t)row * a.k + r] = bi < (float)V ? (int)bi : 0;
    }
    lv = bv; li = bi;
  }
}

// dynamic LDS of a selection launch, or -1 when the row does not fit
int sel_lds_bytes(int V, int n_prev, float penalty) {
  const int64_t need = ((int64_t)V + (penalty != 1.0f ? n_prev : 0)) * 4;
  return need > kSelLdsBytes ? -1 : (int)((need + 15) & ~(int64_t)15);
}

}  // namespace

extern "C" int stllm_select_tokens(const stllm_select_args* a, void* stream) {
  STLLM_CHECK_ARG(a != nullptr, "stllm_select_tokens: null args");
  STLLM_CHECK_ARG(a->logits && a->out && a->rows > 0 && a->V > 0 && a->ldl >= a->V, "stllm_select_tokens: bad logits / out / rows=%d V=%d ldl=%lld", a->rows,
                  a->V, (long long)a->ldl);
  STLLM_CHECK_ARG(a->n_prev >= 0 && (a->n_prev == 0 || (a->prev && a->ld_prev >= a->n_prev)), "stllm_select_tokens: prev needs n_prev <= ld_prev");
  STLLM_CHECK_ARG(a->penalty > 0.0f, "stllm_select_tokens: penalty must be positive");
  STLLM_CHECK_ARG(!a->sample || (a->u && a->temperature > 0.0f && a->top_p > 0.0f), "stllm_select_tokens(sample): needs u, temperature > 0, top_p > 0");
  const int lds = sel_lds_bytes(a->V, a->n_prev, a->penalty);
  if (lds < 0) {
    stllm_set_error("stllm_select_tokens: V=%d (+ n_prev=%d) floats do not fit %d bytes of LDS", a->V, a->n_prev, kSelLdsBytes);
    return STLLM_ERR_UNSUPPORTED;
  }
  static StllmPerDevice lds_dev;   // largest dynamic-LDS size opted into, per device ordinal
  bool lds_first;
  const int lds_d = lds_dev.enter(&lds_first);
  if (lds_first || lds > lds_dev.value[lds_d]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(select_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
      stllm_set_error("stllm_select_tokens: cannot opt into %d bytes of LDS", lds);
      return STLLM_ERR_UNSUPPORTED;
    }
    lds_dev.value[lds_d] = lds;
    lds_dev.done(lds_d);
  }
  hipLaunchKernelGGL(select_kernel<false>, dim3(a->rows), dim3(kSelThreads), lds, reinterpret_cast<hipStream_t>(stream), *a);
  STLLM_CHECK_LAUNCH("stllm_select_tokens");
  return STLLM_OK;
}

extern "C" int stllm_beam_candidates(const stllm_beam_args* a, void* stream) {
  STLLM_CHECK_ARG(a != nullptr, "stllm_beam_candidates: null args");
  STLLM_CHECK_ARG(a->logits && a->beam_score && a->cand_score && a->cand_token && a->rows > 0 && a->V > 0 && a->ldl >= a->V,
                  "stllm_beam_candidates: bad pointers / rows=%d V=%d ldl=%lld", a->rows, a->V, (long long)a->ldl);
  STLLM_CHECK_ARG(a->k >= 1 && a->k <= 32 && a->k <= a->V, "stllm_beam_candidates: 1 <= k=%d <= min(32, V=%d)", a->k, a->V);
  STLLM_CHECK_ARG(a->n_prev >= 0 && (a->n_prev == 0 || (a->prev && a->ld_prev >= a->n_prev)), "stllm_beam_candidates: prev needs n_prev <= ld_prev");
  STLLM_CHECK_ARG(a->penalty > 0.0f, "stllm_beam_candidates: penalty must be positive");
  const int lds = sel_lds_bytes(a->V, a->n_prev, a->penalty);
  if (lds < 0) {
    stllm_set_error("stllm_beam_candidates: V=%d (+ n_prev=%d) floats do not fit %d bytes of LDS", a->V, a->n_prev, kSelLdsBytes);
    return STLLM_ERR_UNSUPPORTED;
  }
  static StllmPerDevice lds_dev;   // largest dynamic-LDS size opted into, per device ordinal
  bool lds_first;
  const int lds_d = lds_dev.enter(&lds_first);
  if (lds_first || lds > lds_dev.value[lds_d]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(beam_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
      stllm_set_error("stllm_beam_candidates: cannot opt into %d bytes of LDS", lds);
      return STLLM_ERR_UNSUPPORTED;
    }
    lds_dev.value[lds_d] = lds;
    lds_dev.done(lds_d);
  }
  hipLaunchKernelGGL(beam_kernel<false>, dim3(a->rows), dim3(kSelThreads), lds, reinterpret_cast<hipStream_t>(stream), *a);
  STLLM_CHECK_LAUNCH("stllm_beam_candidates");
  return STLLM_OK;
}

extern "C" int stllm_beam_candidates_rows(const stllm_beam_rows_args* a, void* stream) {
  STLLM_CHECK_ARG(a != nullptr, "stllm_beam_candidates_rows: null args");
  STLLM_CHECK_ARG(a->logits && a->beam_score && a->cand_score && a->cand_token && a->n_logits_rows > 0 && a->V > 0 && a->ldl >= a->V,
                  "stllm_beam_candidates_rows: bad pointers / n_logits_rows=%d V=%d ldl=%lld", a->n_logits_rows, a->V, (long long)a->ldl);
  STLLM_CHECK_ARG(a->rows > 0 && a->src && a->n_prev, "stllm_beam_candidates_rows: bad src / n_prev / rows=%d", a->rows);
  STLLM_CHECK_ARG(a->k >= 1 && a->k <= 32 && a->k <= a->V, "stllm_beam_candidates_rows: 1 <= k=%d <= min(32, V=%d)", a->k, a->V);
  STLLM_CHECK_ARG(a->ld_prev >= 0 && (a->ld_prev == 0 || a->prev), "stllm_beam_candidates_rows: prev needs ld_prev >= 0 (NULL only with ld_prev == 0)");
  STLLM_CHECK_ARG(a->penalty > 0.0f, "stllm_beam_candidates_rows: penalty must be positive");
  const int64_t need = ((int64_t)a->V + a->ld_prev) * 4;   // the row and a whole history, whatever the rows hold in this step
  if (need > kSelLdsBytes) {
    stllm_set_error("stllm_beam_candidates_rows: V=%d + ld_prev=%lld floats do not fit %d bytes of LDS", a->V, (long long)a->ld_prev, kSelLdsBytes);
    return STLLM_ERR_UNSUPPORTED;
  }
  const int lds = (int)((need + 15) & ~(int64_t)15);
  static StllmPerDevice lds_dev;   // largest dynamic-LDS size opted into, per device ordinal
  bool lds_first;
  const int lds_d = lds_dev.enter(&lds_first);
  if (lds_first || lds > lds_dev.value[lds_d]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(beam_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
      stllm_set_error("stllm_beam_candidates_rows: cannot opt into %d bytes of LDS", lds);
      return STLLM_ERR_UNSUPPORTED;
    }
    lds_dev.value[lds_d] = lds;
    lds_dev.done(lds_d);
  }
  hipLaunchKernelGGL(beam_kernel<true>, dim3(a->rows), dim3(kSelThreads), lds, reinterpret_cast<hipStream_t>(stream), *a);
  STLLM_CHECK_LAUNCH("stllm_beam_candidates_rows");
  return STLLM_OK;
}

extern "C" int stllm_kv_reorder_rows(int dtype, void* cache, int64_t batch_stride, int64_t row_stride, const int32_t* src, const int32_t* lo,
                                     const int32_t* hi, int rows, int nb, int hidden, int capacity, int max_span, void* stream) {
  STLLM_CHECK_ARG(cache && src && lo && hi, "stllm_kv_reorder_rows: null pointer");
  STLLM_CHECK_ARG(rows > 0 && nb >= 1 && rows % nb == 0 && rows / nb <= 65535 && hidden > 0 && capacity > 0 && max_span > 0,
                  "stllm_kv_reorder_rows: bad rows=%d nb=%d hidden=%d capacity=%d max_span=%d (rows a multiple of nb, rows / nb <= 65535)", rows, nb, hidden,
                  capacity, max_span);
  if (nb > kReorderMaxBeams) {
    stllm_set_error("stllm_kv_reorder_rows: nb=%d rows per group, at most %d are held in registers", nb, kReorderMaxBeams);
    return STLLM_ERR_UNSUPPORTED;
  }
  int e;
  switch (dtype) {
    case STLLM_BF16: case STLLM_F16: e = 2; break;
    case STLLM_F32: e = 4; break;
    default: stllm_set_error("stllm_kv_reorder_rows: bad dtype %d", dtype); return STLLM_ERR_BAD_DTYPE;
  }
  STLLM_CHECK_ARG(row_stride >= 3 * (int64_t)hidden && batch_stride >= (int64_t)capacity * row_stride,
                  "stllm_kv_reorder_rows: rows of 3 * hidden elements, capacity rows per cache row");
  STLLM_CHECK_ARG(((int64_t)hidden * e) % 16 == 0 && (row_stride * e) % 16 == 0 && (batch_stride * e) % 16 == 0 && aligned16(cache) &&
                      ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(hi)) & 3) == 0,
                  "stllm_kv_reorder_rows: 16-byte vector copies need 16-byte aligned pointers, strides and hidden");
  const int col0 = hidden * e, n16 = (2 * hidden * e) / 16;
  const int64_t cells = (int64_t)(max_span < capacity ? max_span : capacity) * n16;
  hipLaunchKernelGGL(kv_reorder_rows_kernel, dim3((unsigned)((cells + 255) / 256), rows / nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<char*>(cache), batch_stride * e, row_stride * e, src, lo, hi, nb, capacity, col0, n16);
  STLLM_CHECK_LAUNCH("stllm_kv_reorder_rows");
  return STLLM_OK;
}

extern "C" int stllm_select_slots(const stllm_select_slots_args* a, void* stream) {
  STLLM_CHECK_ARG(a != nullptr, "stllm_select_slots: null args");
  STLLM_CHECK_ARG(a->logits && a->rows > 0 && a->V > 0 && a->ldl >= a->V, "stllm_select_slots: bad logits / rows=%d V=%d ldl=%lld", a->rows, a->V,
                  (long long)a->ldl);
  STLLM_CHECK_ARG(a->n_slots > 0 && a->src && a->state && a->ids && a->ld_ids >= 1, "stllm_select_slots: bad src / state / ids / n_slots=%d ld_ids=%lld",
                  a->n_slots, (long long)a->ld_ids);
  STLLM_CHECK_ARG(a->n_stop >= 0 && (a->n_stop == 0 || (a->stops && a->stop_len && a->ld_stop >= 1)), "stllm_select_slots: stops needs stop_len and ld_stop >= 1");
  STLLM_CHECK_ARG(a->penalty > 0.0f, "stllm_select_slots: penalty must be positive");
  STLLM_CHECK_ARG(!a->sample || (a->u && a->temperature > 0.0f && a->top_p > 0.0f), "stllm_select_slots(sample): needs u, temperature > 0, top_p > 0");
  const int64_t need = ((int64_t)a->V + a->ld_ids) * 4;   // the row and a whole history, whatever the slots hold in this step
  if (need > kSelLdsBytes) {
    stllm_set_error("stllm_select_slots: V=%d + ld_ids=%lld floats do not fit %d bytes of LDS", a->V, (long long)a->ld_ids, kSelLdsBytes);
    return STLLM_ERR_UNSUPPORTED;
  }
  const int lds = (int)((need + 15) & ~(int64_t)15);
  static StllmPerDevice lds_dev;   // largest dynamic-LDS size opted into, per device ordinal
  bool lds_first;
  const int lds_d = lds_dev.enter(&lds_first);
  if (lds_first || lds > lds_dev.value[lds_d]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(select_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
      stllm_set_error("stllm_select_slots: cannot opt into %d bytes of LDS", lds);
      return STLLM_ERR_UNSUPPORTED;
    }
    lds_dev.value[lds_d] = lds;
    lds_dev.done(lds_d);
  }
  hipLaunchKernelGGL(select_kernel<true>, dim3(a->n_slots), dim3(kSelThreads), lds, reinterpret_cast<hipStream_t>(stream), *a);
  STLLM_CHECK_LAUNCH("stllm_select_slots");
  return STLLM_OK;
}

extern "C" int stllm_kv_append_rows(int dtype, const void* src, int64_t ld_src, void* cache, int64_t batch_stride, int64_t row_stride,
                                    const int32_t* pos, int B, int hidden, int max_len, int with_q, void* stream) {
  STLLM_CHECK_ARG(src && cache && pos, "stllm_kv_append_rows: null pointer");
  STLLM_CHECK_ARG(B > 0 && hidden > 0 && max_len > 0, "stllm_kv_append_rows: bad B=%d hidden=%d max_len=%d", B, hidden, max_len);
  int e;
  switch (dtype) {
    case STLLM_BF16: case STLLM_F16: e = 2; break;
    case STLLM_F32: e = 4; break;
    default: stllm_set_error("stllm_kv_append_rows: bad dtype %d", dtype); return STLLM_ERR_BAD_DTYPE;
  }
  STLLM_CHECK_ARG(ld_src >= 3 * (int64_t)hidden && row_stride >= 3 * (int64_t)hidden && batch_stride >= (int64_t)max_len * row_stride,
                  "stllm_kv_append_rows: rows of 3 * hidden elements, max_len rows per batch entry");
  STLLM_CHECK_ARG(((int64_t)hidden * e) % 16 == 0 && (ld_src * e) % 16 == 0 && (row_stride * e) % 16 == 0 && (batch_stride * e) % 16 == 0 &&
                      aligned16(src) && aligned16(cache) && (reinterpret_cast<uintptr_t>(pos) & 3) == 0,
                  "stllm_kv_append_rows: 16-byte vector copies need 16-byte aligned pointers, strides and hidden");
  const int col0 = with_q ? 0 : hidden * e, n16 = (3 * hidden * e - col0) / 16;
  hipLaunchKernelGGL(kv_append_rows_kernel, dim3((n16 + 255) / 256, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const char*>(src), ld_src * e, reinterpret_cast<char*>(cache), batch_stride * e, row_stride * e, pos, max_len, col0, n16);
  STLLM_CHECK_LAUNCH("stllm_kv_append_rows");
  return STLLM_OK;
}

extern "C" int stllm_kv_append_spans(int dtype, const void* src, int64_t ld_src, void* cache, int64_t batch_stride, int64_t row_stride,
                                     const int32_t* pos0, const int32_t* n, int B, int S, int hidden, int max_len, void* stream) {
  STLLM_CHECK_ARG(src && cache && pos0 && n, "stllm_kv_append_spans: null pointer");
  STLLM_CHECK_ARG(B > 0 && S > 0 && hidden > 0 && max_len > 0 && (int64_t)B * S <= 65535, "stllm_kv_append_spans: bad B=%d S=%d hidden=%d max_len=%d (B * S <= 65535)",
                  B, S, hidden, max_len);
  int e;
  switch (dtype) {
    case STLLM_BF16: case STLLM_F16: e = 2; break;
    case STLLM_F32: e = 4; break;
    default: stllm_set_error("stllm_kv_append_spans: bad dtype %d", dtype); return STLLM_ERR_BAD_DTYPE;
  }
  STLLM_CHECK_ARG(ld_src >= 3 * (int64_t)hidden && row_stride >= 3 * (int64_t)hidden && batch_stride >= (int64_t)max_len * row_stride,
                  "stllm_kv_append_spans: rows of 3 * hidden elements, max_len rows per batch entry");
  STLLM_CHECK_ARG(((int64_t)hidden * e) % 16 == 0 && (ld_src * e) % 16 == 0 && (row_stride * e) % 16 == 0 && (batch_stride * e) % 16 == 0 &&
                      aligned16(src) && aligned16(cache) && (reinterpret_cast<uintptr_t>(pos0) & 3) == 0 && (reinterpret_cast<uintptr_t>(n) & 3) == 0,
                  "stllm_kv_append_spans: 16-byte vector copies need 16-byte aligned pointers, strides and hidden");
  const int col0 = hidden * e, n16 = (2 * hidden * e) / 16;
  hipLaunchKernelGGL(kv_append_spans_kernel, dim3((n16 + 255) / 256, B * S), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const char*>(src), ld_src * e, reinterpret_cast<char*>(cache), batch_stride * e, row_stride * e, pos0, n, S, max_len, col0,
                     n16);
  STLLM_CHECK_LAUNCH("stllm_kv_append_spans");
  return STLLM_OK;
}

extern "C" int stllm_kv_append_segments(int dtype, const void* src, int64_t ld_src, void* cache, int64_t batch_stride, int64_t row_stride,
                                        const int32_t* slot, const int32_t* row0, const int32_t* pos0, const int32_t* n, int R, int T, int n_slots,
                                        int max_n, int hidden, int max_len, void* stream) {
  STLLM_CHECK_ARG(src && cache && slot && row0 && pos0 && n, "stllm_kv_append_segments: null pointer");
  STLLM_CHECK_ARG(R > 0 && R <= 65535 && T > 0 && n_slots > 0 && max_n > 0 && max_n <= 65535 && hidden > 0 && max_len > 0,
                  "stllm_kv_append_segments: bad R=%d T=%d n_slots=%d max_n=%d hidden=%d max_len=%d (R, max_n <= 65535)", R, T, n_slots, max_n, hidden, max_len);
  int e;
  switch (dtype) {
    case STLLM_BF16: case STLLM_F16: e = 2; break;
    case STLLM_F32: e = 4; break;
    default: stllm_set_error("stllm_kv_append_segments: bad dtype %d", dtype); return STLLM_ERR_BAD_DTYPE;
  }
  STLLM_CHECK_ARG(ld_src >= 3 * (int64_t)hidden && row_stride >= 3 * (int64_t)hidden && batch_stride >= (int64_t)max_len * row_stride,
                  "stllm_kv_append_segments: rows of 3 * hidden elements, max_len rows per cache row");
  STLLM_CHECK_ARG(((int64_t)hidden * e) % 16 == 0 && (ld_src * e) % 16 == 0 && (row_stride * e) % 16 == 0 && (batch_stride * e) % 16 == 0 &&
                      aligned16(src) && aligned16(cache) &&
                      ((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(row0) | reinterpret_cast<uintptr_t>(pos0) |
                        reinterpret_cast<uintptr_t>(n)) & 3) == 0,
                  "stllm_kv_append_segments: 16-byte vector copies need 16-byte aligned pointers, strides and hidden");
  const int col0 = hidden * e, n16 = (2 * hidden * e) / 16;
  hipLaunchKernelGGL(kv_append_segments_kernel, dim3((n16 + 255) / 256, max_n, R), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const char*>(src), ld_src * e, reinterpret_cast<char*>(cache), batch_stride * e, row_stride * e, slot, row0, pos0, n, T,
                     n_slots, max_len, col0, n16);
  STLLM_CHECK_LAUNCH("stllm_kv_append_segments");
  return STLLM_OK;
}

extern "C" int stllm_gather_rows(const float* src_a, int64_t ld_a, const float* src_b, int64_t ld_b,
                                 const int32_t* idx_a, const float* add, int64_t ld_add, const int32_t* idx_add,
                                 float* dst, int64_t ld_dst, int n_rows, int D, float scale, void* stream) {
  STLLM_CHECK_ARG(src_a && idx_a && dst, "stllm_gather_rows: null pointer");
  STLLM_CHECK_ARG(n_rows > 0 && D > 0 && D % 4 == 0, "stllm_gather_rows: bad n_rows=%d D=%d", n_rows, D);
  STLLM_CHECK_ARG(ld_a % 4 == 0 && ld_dst % 4 == 0 && aligned16(src_a) && aligned16(dst), "stllm_gather_rows: misaligned");
  STLLM_CHECK_ARG(!src_b || (ld_b % 4 == 0 && aligned16(src_b)), "stllm_gather_rows: src_b misaligned");
  STLLM_CHECK_ARG(!add || (idx_add && ld_add % 4 == 0 && aligned16(add)), "stllm_gather_rows: add needs idx_add, aligned");
  hipLaunchKernelGGL(gather_rows_kernel, dim3(n_rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src_a, ld_a,
                     src_b, ld_b, idx_a, add, ld_add, idx_add, dst, ld_dst, n_rows, D, scale);
  STLLM_CHECK_LAUNCH("stllm_gather_rows");
  return STLLM_OK;
}

extern "C" int stllm_mean_t(const float* x, float* out, int B, int T, int64_t J, void* stream) {
  STLLM_CHECK_ARG(x && out && B > 0 && T > 0 && J > 0 && J % 4 == 0, "stllm_mean_t: bad args");
  STLLM_CHECK_ARG(aligned16(x) && aligned16(out), "stllm_mean_t: misaligned");
  const int64_t J4 = J / 4;
  hipLaunchKernelGGL(mean_t_kernel, dim3((unsigned)((J4 + 255) / 256), B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, out, T, J4);
  STLLM_CHECK_LAUNCH("stllm_mean_t");
  return STLLM_OK;
}

extern "C" int stllm_vit_cls_rows(const float* cls, const float* pos, float* x, int64_t ldx, int n_frames, int D,
                                  void* stream) {
  STLLM_CHECK_ARG(cls && pos && x && n_frames > 0 && D > 0, "stllm_vit_cls_rows: bad args");
  hipLaunchKernelGGL(cls_rows_kernel, dim3(n_frames), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), cls, pos, x,
                     ldx, D);
  STLLM_CHECK_LAUNCH("stllm_vit_cls_rows");
  return STLLM_OK;
}

extern "C" int stllm_cosine_rows(const float* a, int64_t lda, const int32_t* idx_a, const float* b, int64_t ldb,
                                 const int32_t* idx_b, float* out, int n_rows, int D, void* stream) {
  STLLM_CHECK_ARG(a && b && out && n_rows > 0 && D > 0 && D % 4 == 0, "stllm_cosine_rows: bad args");
  STLLM_CHECK_ARG(lda % 4 == 0 && ldb % 4 == 0 && aligned16(a) && aligned16(b), "stllm_cosine_rows: misaligned");
  hipLaunchKernelGGL(cosine_rows_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a,
                     lda, idx_a, b, ldb, idx_b, out, n_rows, D);
  STLLM_CHECK_LAUNCH("stllm_cosine_rows");
  return STLLM_OK;
}

extern "C" int stllm_cross_entropy_rows(const float* logits, int64_t ldl, const int32_t* labels, float* loss,
                                        int n_rows, int V, void* stream) {
  STLLM_CHECK_ARG(logits && labels && loss && n_rows > 0 && V > 0, "stllm_cross_entropy_rows: bad args");
  hipLaunchKernelGGL(ce_rows_kernel, dim3(n_rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), logits, ldl,
                     labels, loss, V);
  STLLM_CHECK_LAUNCH("stllm_cross_entropy_rows");
  return STLLM_OK;
}

extern "C" int stllm_cast_rows(int dtype, const float* x, int64_t ldx, void* out, int64_t ldo, int M, int D,
                               void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(x && out && M > 0 && D > 0 && D % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0, "stllm_cast_rows: bad args");
  STLLM_CHECK_ARG(aligned16(x) && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "stllm_cast_rows: misaligned");
  switch (dtype) {
    case STLLM_BF16: hipLaunchKernelGGL(cast_rows_kernel<bf16_t>, dim3(M), dim3(256), 0, stream, x, ldx, out, ldo, D); break;
    case STLLM_F16: hipLaunchKernelGGL(cast_rows_kernel<f16_t>, dim3(M), dim3(256), 0, stream, x, ldx, out, ldo, D); break;
    case STLLM_F32: hipLaunchKernelGGL(cast_rows_kernel<float>, dim3(M), dim3(256), 0, stream, x, ldx, out, ldo, D); break;
    default: stllm_set_error("stllm_cast_rows: bad dtype %d", dtype); return STLLM_ERR_BAD_DTYPE;
  }
  STLLM_CHECK_LAUNCH("stllm_cast_rows");
  return STLLM_OK;
}
