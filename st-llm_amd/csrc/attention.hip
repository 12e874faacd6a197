// Fused attention  out = softmax(scale * Q K^T + mask) V   (never materialises S)
//
// 16-bit path (bf16/fp16, MFMA 32x32x16, fp32 online softmax) — "everything transposed" layout:
//   * a wave owns 32 query rows; a workgroup = NW waves = 32*NW rows of one (batch, head).
//   * per 32-key tile:  S^T[kv][q] = K_tile[kv][d] . Q^T[d][q]      (A = K from LDS, B = Q in VGPRs)
//     so every lane holds 16 scores of ONE query (q = lane & 31): row max / row sum are in-lane
//     reductions plus a single lane<->lane+32 exchange (wave shuffles), no LDS round trip.
//   * P^T stays in registers and is already in B-operand form for
//                         O^T[d][q] += V^T[d][kv] . P^T[kv][q]       (A = V^T from LDS)
//     the key<->k-slot map of the MFMA is free as long as A and B agree, so the S^T accumulator
//     register order {0-3,8-11 | 4-7,12-15}+16a is used as the contraction order directly: V^T
//     fragments are two 8-byte LDS reads at [d][16a+4h] and [d][16a+8+4h].
//   * O^T columns are queries too, so the online-softmax rescale is an in-lane multiply.
//   * K tile rows are padded by 16 B and V^T rows by 8 B: conflict-free ds_read_b128 / ds_read_b64.
//   * head_dim 88 (EVA-CLIP-g) is zero-padded to 96 in LDS/registers only; HBM traffic stays 88.
// fp32 path ("verify" numerics): attn_mfma_f32_kernel — the same schedule on exact-fp32 MFMAs (32x32x2) — from 8 query rows on; an
// exact-fp32 vector kernel, one wave per query row, for the one-row decode step.
#include <cstdlib>
#include "common.h"

namespace {

struct AttnParams {
  const char* q; int64_t q_bs, q_rs;   // strides in elements
  const char* k; int64_t k_bs, k_rs;
  const char* v; int64_t v_bs, v_rs;
  char* o; int64_t o_bs, o_rs;
  int B, H, Sq, Skv, D;
  float scale_log2;                     // scale * log2(e)
  float scale;
  int causal;
  const int32_t* kv_len;
  int q_lds;                            // attn_dma_kernel: the query tiles arrive through the LDS (set by launch_dma when they fit)
  int merge_par;                        // attn_dma_kernel, KS2 > 1: every partner wave has its own merge slot (one barrier pair instead of one per partner)
  // stllm_attention_offset (0 / null through stllm_attention): query row i sits at position q_off + i, so with `causal` key j is visible iff j <= q_off + i.
  // Read by attn_mfma_kernel, attn_mfma_f32_kernel and attn_f32_kernel only; the LDS-DMA / resident kernels are not reached with an offset.
  int q_off;
  float* ws; int nsplit, kps;           // attn_mfma_kernel<.., SPLIT>: partial records, key ranges per query chunk, keys per range (a multiple of 32)
};

// stllm_attention_offset_ragged: the RAGGED instantiations take the query offset PER BATCH ROW on top (with kv_len: row b holds q_off_tab[b] cached positions
// and kv_len[b] - q_off_tab[b] new ones).  A type of its own, so that the kernel arguments of every other instantiation stay what they were.
struct AttnRaggedParams : AttnParams { const int32_t* q_off_tab; };
// stllm_attention_segments: the SEG instantiations (RAGGED on top) read a PACKED query buffer: "batch row" r is a segment whose K / V sit in cache row slot[r]
// and whose n_r query / output rows are the packed rows row0[r] .. row0[r] + n_r - 1 (q_bs / o_bs unused: the bases are row0[r] * q_rs / o_rs); T packed
// rows, n_slots cache rows.  Again a type of its own: the arguments of every other instantiation stay what they were.
struct AttnSegParams : AttnRaggedParams { const int32_t* slot; const int32_t* row0; int T, n_slots; };
template <bool RAGGED, bool SEG = false> struct AttnParamsOf { using type = AttnParams; };
template <> struct AttnParamsOf<true, false> { using type = AttnRaggedParams; };
template <> struct AttnParamsOf<true, true> { using type = AttnSegParams; };

// the per-row tables of the RAGGED instantiations, clamped: 0 <= q_off <= kvlen <= Skv and n = kvlen - q_off <= Sq new rows.  A row without new positions
// (n == 0) gets kvlen = 0: its workgroups walk no key and load nothing.  b is workgroup-uniform, so all three live in scalar registers.
struct RaggedRow { int q_off, kvlen, n; };
__device__ __forceinline__ RaggedRow ragged_row(const AttnRaggedParams& p, int b) {
  RaggedRow r;
  const int len = max(min(p.kv_len[b], p.Skv), 0);
  r.q_off = max(min(p.q_off_tab[b], len), 0);
  r.n = min(len - r.q_off, p.Sq);
  r.kvlen = r.n > 0 ? r.q_off + r.n : 0;
  return r;
}
// ... and what every other instantiation has always used, in the same shape
__device__ __forceinline__ RaggedRow ragged_row(const AttnParams& p, int b) {
  return RaggedRow{p.q_off, p.kv_len ? min(p.kv_len[b], p.Skv) : p.Skv, p.Sq};
}

// a segment of the SEG instantiations: ragged_row's clamps, then the table guard — a slot outside [0, n_slots) or packed rows outside [0, T) make the segment
// empty (n = 0, kvlen = 0: its workgroups walk no key, load nothing and store nothing), so that a bad table cannot reach memory outside the buffers.
struct SegRow : RaggedRow { int slot, row0; };
__device__ __forceinline__ SegRow seg_row(const AttnSegParams& p, int r) {
  SegRow s;
  static_cast<RaggedRow&>(s) = ragged_row(static_cast<const AttnRaggedParams&>(p), r);
  s.slot = p.slot[r];
  s.row0 = p.row0[r];
  if (s.slot < 0 || s.slot >= p.n_slots || s.row0 < 0 || (int64_t)s.row0 + s.n > p.T) { s.n = 0; s.kvlen = 0; s.slot = 0; s.row0 = 0; }
  return s;
}
// where a batch row's K / V, query and output rows start (batch index / elements) and how many query rows exist in memory: the batch strides for every
// instantiation but SEG, the segment's tables for SEG.  Used in place, where the addresses are formed, so that the code of the other instantiations stays what it was.
template <typename P> __device__ __forceinline__ int attn_kv_row(const P&, RaggedRow, int b) { return b; }
template <typename P> __device__ __forceinline__ int attn_kv_row(const P&, SegRow s, int) { return s.slot; }
template <typename P> __device__ __forceinline__ int64_t attn_q_base(const P& p, RaggedRow, int b) { return (int64_t)b * p.q_bs; }
template <typename P> __device__ __forceinline__ int64_t attn_q_base(const P& p, SegRow s, int) { return (int64_t)s.row0 * p.q_rs; }
template <typename P> __device__ __forceinline__ int64_t attn_o_base(const P& p, RaggedRow, int b) { return (int64_t)b * p.o_bs; }
template <typename P> __device__ __forceinline__ int64_t attn_o_base(const P& p, SegRow s, int) { return (int64_t)s.row0 * p.o_rs; }
template <typename P> __device__ __forceinline__ int attn_q_rows(const P& p, RaggedRow) { return p.Sq; }
template <typename P> __device__ __forceinline__ int attn_q_rows(const P&, SegRow s) { return s.n; }

constexpr float kNeg = -1.0e30f;

// in-kernel timeline (tools/attn_trace.sh builds st-llm_amd/attn_trace/libstllm_hip.so with -DSTLLM_ATTN_TRACE; never in the shipped library):
// lane 0 of every wave stamps s_memtime into 8 slots of g_attn_trace[workgroup][wave]; tools/attn_trace.py reads them back.
#ifdef STLLM_ATTN_TRACE
__device__ unsigned long long g_attn_trace[512 * 12 * 8];
#define ATTN_STAMP(slot) do { if ((threadIdx.x & 63) == 0) g_attn_trace[((size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * 12 + (threadIdx.x >> 6)) * 8 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#define ATTN_STAMP_VAL(slot, val) do { if ((threadIdx.x & 63) == 0) g_attn_trace[((size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * 12 + (threadIdx.x >> 6)) * 8 + (slot)] = (unsigned long long)(val); } while (0)
#else
#define ATTN_STAMP(slot) do { } while (0)
#define ATTN_STAMP_VAL(slot, val) do { } while (0)
#endif

// XCD-aware (batch, head, query-chunk) assignment.  The hardware deals workgroups round-robin over the 8 XCDs, each with its own
// L2; with the natural order neighbouring heads of a frame (whose 176-byte K / V rows share cache lines at head_dim 88) and the
// query chunks of one head (which re-read the same K / V) land on DIFFERENT XCDs, and every line is fetched 2-5 times from the
// fabric — the ViT attention spent 38 % of its 26 us waiting for its first 36 KB (timeline: tools/attn_probe.hip).  The bijective
// remap makes the linear ids that one XCD sees consecutive: all chunks of a head, then the next head of the same (frame, batch).
__device__ __forceinline__ void attn_block_coords(int& chunk_x, int& h, int& b) {
  const int gx = gridDim.x, gy = gridDim.y, n = gx * gy * gridDim.z;
  const int lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  const int q = n >> 3, r = n & 7, xcd = lin & 7, k = lin >> 3;
  const int id = ((xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  chunk_x = id % gx;
  h = (id / gx) % gy;
  b = id / (gx * gy);
}

// SPLIT (key-split partial pass of stllm_attention_offset, DP = 128): blockIdx.x = query chunk * nsplit + key range; the workgroup walks the keys
// [range * kps, (range + 1) * kps) only and leaves the un-normalised fp32 state (O[128], m, l) of every query row in p.ws for attn_ksplit_merge_kernel.
constexpr int kSplRec = 132;   // floats per partial record: O[128], m (raw-score maximum), l, 2 pad (16-byte aligned records)

// LIVE (the suffix pass of stllm_attention_shared only): key rows at or behind the batch row's kv_len are not LOADED (zeros instead) — the rows behind a
// suffix's length are uninitialised memory, and a masked score of 0 times a NaN in V would reach the output.  Every other instantiation has LIVE = false
// and compiles to what it always was.
// SEG (stllm_attention_segments, RAGGED on top): blockIdx.z is a segment of a packed query buffer.  A pad query row (i >= n_r) does not exist there — packed row
// row0 + i belongs to another segment or lies behind T —, so it is neither loaded (zeros) nor stored, as output or as a key-split record.
template <typename T, int DP, int NW, bool SPLIT = false, bool LIVE = false, bool RAGGED = false, bool SEG = false>
__global__ __launch_bounds__(64 * NW) void attn_mfma_kernel(const typename AttnParamsOf<RAGGED, SEG>::type p) {
  constexpr int KS = DP / 16;          // k-steps of the S^T MFMA chain
  constexpr int DB = DP / 32;          // 32-row blocks of O^T
  constexpr int KPITCH = DP * 2 + 16;  // bytes per K row in LDS
  constexpr int VPITCH = 32 * 2 + 8;   // bytes per V^T row in LDS
  constexpr int NT = 64 * NW;
  constexpr int CPR = DP / 8;          // 16-byte chunks per K/V row
  constexpr int NCH = 32 * CPR;        // chunks per tile
  constexpr int CPT = (NCH + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) char k_lds[32 * KPITCH];
  __shared__ __attribute__((aligned(16))) char v_lds[DP * VPITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q_chunk = SPLIT ? (int)blockIdx.x / p.nsplit : (int)blockIdx.x;
  const int k_range = SPLIT ? (int)blockIdx.x - q_chunk * p.nsplit : 0;
  const int q_blk0 = q_chunk * (32 * NW);
  const int qrow = q_blk0 + wave * 32 + li;  // this lane's query
  const int D = p.D;
  static_assert(!RAGGED || LIVE, "the rows behind a ragged row's length are uninitialised: live loads only");
  static_assert(!SEG || RAGGED, "segments are ragged rows of a packed buffer");
  const auto rr = [&] { if constexpr (SEG) return seg_row(p, b); else return ragged_row(p, b); }();
  const int kvlen = rr.kvlen;
  // the query offset, read where it is used: per batch row (RAGGED) or the call's (every other instantiation, whose code this keeps what it was)
#define ATTN_Q_OFF (RAGGED ? rr.q_off : p.q_off)
  const int n_new = rr.n;       // the live query rows of this batch row (RAGGED; the rows behind them are pad and come out as zeros)

  // ---- Q fragments (B operand of S^T): lane holds Q[q][ks*16 + lh*8 .. +8] ------------------------
  i32x4 qf[KS];
  {
    const char* qp = p.q + (attn_q_base(p, rr, b) + (int64_t)(qrow < attn_q_rows(p, rr) ? qrow : 0) * p.q_rs + (int64_t)h * D) * 2;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = ks * 16 + lh * 8;
      i32x4 z = {0, 0, 0, 0};
      qf[ks] = (qrow < attn_q_rows(p, rr) && d0 < D) ? *reinterpret_cast<const i32x4*>(qp + d0 * 2) : z;
    }
  }

  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.0f;
  float m_run = kNeg, l_run = 0.0f;

  int kv_end = kvlen;
  if (p.causal) kv_end = min(kv_end, ATTN_Q_OFF + q_blk0 + 32 * NW);  // keys beyond the last query of the block are masked
  const int kv_begin = SPLIT ? k_range * p.kps : 0;
  if (SPLIT) kv_end = min(kv_end, kv_begin + p.kps);
  if constexpr (RAGGED) {
    if (q_blk0 >= n_new) kv_end = 0;   // every query row of this workgroup is pad: it walks no key, loads nothing and stores its zeros / empty records
  }
  const char* kbase = p.k + ((int64_t)attn_kv_row(p, rr, b) * p.k_bs + (int64_t)h * D) * 2;
  const char* vbase = p.v + ((int64_t)attn_kv_row(p, rr, b) * p.v_bs + (int64_t)h * D) * 2;

  // K/V tiles are register-staged one tile AHEAD: the global loads of tile t+1 are issued before the MFMA/softmax work of
  // tile t and only consumed (written to LDS) at the top of the next iteration — HBM/L2 latency hides under compute.
  i32x4 kreg[CPT], vreg[CPT];
  auto load_tile = [&](int kv0) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int ch = tid + c * NT;
      const int cc = ch >> 5, row = ch & 31;   // consecutive lanes = consecutive keys: conflict-free transposed V writes
      const int kv = kv0 + row;
      const bool ok = (ch < NCH) && (kv < (LIVE ? kvlen : p.Skv)) && (cc * 8 < D);
      i32x4 z = {0, 0, 0, 0};
      kreg[c] = ok ? *reinterpret_cast<const i32x4*>(kbase + ((int64_t)kv * p.k_rs + cc * 8) * 2) : z;
      vreg[c] = ok ? *reinterpret_cast<const i32x4*>(vbase + ((int64_t)kv * p.v_rs + cc * 8) * 2) : z;
    }
  };
  const int wave_q_last = ATTN_Q_OFF + q_blk0 + wave * 32 + 31;  // position of the last query row of this wave (causal tile skipping)
  if (kv_end > kv_begin) load_tile(kv_begin);
  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += 32) {
    __syncthreads();  // previous tile fully consumed
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int ch = tid + c * NT;
      if (ch < NCH) {
        const int cc = ch >> 5, row = ch & 31;
        *reinterpret_cast<i32x4*>(k_lds + row * KPITCH + cc * 16) = kreg[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t w = (uint32_t)vreg[c][e];
          *reinterpret_cast<uint16_t*>(v_lds + (cc * 8 + 2 * e) * VPITCH + row * 2) = (uint16_t)(w & 0xffff);
          *reinterpret_cast<uint16_t*>(v_lds + (cc * 8 + 2 * e + 1) * VPITCH + row * 2) = (uint16_t)(w >> 16);
        }
      }
    }
    __syncthreads();
    if (kv0 + 32 < kv_end) load_tile(kv0 + 32);
    if (p.causal && kv0 > wave_q_last) continue;  // every key of this tile is in the future of every query of this wave
    if constexpr (RAGGED) {
      // a wave whose 32 query rows are all pad took part in the loads and the barriers and skips the MFMA / softmax work: its rows come out as zeros
      // (tile kernel) or as empty records (key split) whatever its state holds (wave-uniform, like the test above)
      if (q_blk0 + wave * 32 >= n_new) continue;
    }

    // ---- S^T = K . Q^T ------------------------------------------------------------------------------
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const i32x4 kf = *reinterpret_cast<const i32x4*>(k_lds + li * KPITCH + (ks * 2 + lh) * 16);
      s = Elem<T>::mfma(kf, qf[ks], s);
    }
    // ---- mask + online softmax (per-lane query); scores stay RAW, the scale is folded into the exp2 argument ----
    const bool need_mask = (kv0 + 32 > kvlen) || (p.causal && kv0 + 31 > ATTN_Q_OFF + q_blk0 + wave * 32);  // wave-uniform
    if (need_mask) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv = kv0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const bool dead = (kv >= kvlen) || (p.causal && kv > qrow + ATTN_Q_OFF);
        s[r] = dead ? kNeg : s[r];
      }
    }
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);               // running max of RAW scores (scale > 0)
    const float mc = m_new * p.scale_log2;
    float rs = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pv = __builtin_amdgcn_exp2f(fmaf(s[r], p.scale_log2, -mc));   // masked: exp2(-huge) == 0
      s[r] = pv;
      rs += pv;
    }
    rs += __shfl_xor(rs, 32, 64);
    if (__any(m_new != m_run)) {   // rescale only when some query's running max moved (wave-uniform branch)
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
      m_run = m_new;
    }
    l_run += rs;

    // ---- O^T += V^T . P^T ----------------------------------------------------------------------------
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      i32x4 pf;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        pf[e] = (int)(Elem<T>::pack2(s[a * 8 + 2 * e], s[a * 8 + 2 * e + 1]));
#pragma unroll
      for (int i = 0; i < DB; ++i) {
        const char* vp = v_lds + (i * 32 + li) * VPITCH + (16 * a + 4 * lh) * 2;
        const i32x2 lo = *reinterpret_cast<const i32x2*>(vp);
        const i32x2 hi = *reinterpret_cast<const i32x2*>(vp + 16);
        const i32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
        o[i] = Elem<T>::mfma(vf, pf, o[i]);
      }
    }
  }

  // ---- normalise and store: lane holds O[q][d = i*32 + (r&3) + 8*(r>>2) + 4*lh] ------------------------
  if constexpr (SPLIT) {
    static_assert(!SPLIT || DP == 128, "the partial records hold 128 dims");
    if (qrow < attn_q_rows(p, rr)) {   // SEG: a pad row leaves no record (the merge does not read one)
      // a row that saw no key of this range (its tiles skipped, or every key of them masked) has m_run == kNeg and, where a tile was walked for the
      // sake of the wave's other rows, exp2(0) weights in l / O: its record is the empty state, which the merge weighs with exactly 0
      bool empty = m_run <= 0.5f * kNeg;
      if constexpr (RAGGED) empty = empty || qrow >= n_new;   // a pad row's record is empty too (the merge writes its zeros)
      float* rec = p.ws + ((((int64_t)b * p.H + h) * p.Sq + qrow) * p.nsplit + k_range) * kSplRec;
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 ov = {o[i][4 * g + 0], o[i][4 * g + 1], o[i][4 * g + 2], o[i][4 * g + 3]};
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<f32x4*>(rec + i * 32 + 8 * g + 4 * lh) = empty ? z : ov;
        }
      if (lh == 0) { rec[128] = empty ? kNeg : m_run; rec[129] = empty ? 0.0f : l_run; }
    }
    return;
  }
  if (qrow < attn_q_rows(p, rr)) {
    const float inv = 1.0f / l_run;
    uint16_t* op = reinterpret_cast<uint16_t*>(p.o) + attn_o_base(p, rr, b) + (int64_t)qrow * p.o_rs + (int64_t)h * D;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = i * 32 + 8 * g + 4 * lh;
        if (d0 < D) {  // D % 4 == 0
          uint2 pk;
          pk.x = Elem<T>::pack2(o[i][4 * g + 0] * inv, o[i][4 * g + 1] * inv);
          pk.y = Elem<T>::pack2(o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv);
          if constexpr (RAGGED) {
            if (qrow >= n_new) { pk.x = 0u; pk.y = 0u; }   // pad rows are written as exact zeros (their state may hold anything, NaN included)
          }
          *reinterpret_cast<uint2*>(op + d0) = pk;
        }
      }
    }
  }
}
#undef ATTN_Q_OFF

// ---- resident-K/V variant for short key sequences (ViT: 257 keys, Q-Former cross-attention) ----------------
// The whole K (row-major, padded rows) and V^T of one (batch, head) are staged into LDS ONCE (<= 116 KiB for 288 keys x
// 96 dims), one barrier, then every wave walks all key tiles for its own 32 query rows with NO further barriers: waves
// run decoupled, so LDS/MFMA/VALU latencies of one wave hide under the others (PMC on the tiled kernel: 55 % of wave
// time parked at barriers/waits).  One workgroup per (batch, head): 16 frames x 16 heads = 256 workgroups = one per CU.
// KS2 = 2 / 4: every query tile is worked on by KS2 waves that take every KS2-th 32-key tile (the causal prefill has few, long
// query tiles: 32 heads x 18 tiles walk up to 18 key tiles each — the serial walk, not the FLOPs, sets the time); the
// partial (m, l, O) states are merged through LDS at the end.
template <typename T, int DP, int SKV_MAX, int KS2 = 1>
__global__ __launch_bounds__(768) void attn_resident_kernel(const AttnParams p) {
  // SKV_MAX = keys staged per pass (the "window").  Keys beyond one window are handled by further passes (one pair of
  // barriers per window instead of per 32-key tile); blockIdx.x selects a chunk of blockDim.x/64 query tiles.
  constexpr int KS = DP / 16, DB = DP / 32;
  constexpr int KPITCH = DP * 2 + 16;
  constexpr int VPITCH = SKV_MAX * 2 + 8;
  constexpr int CPR = DP / 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;
  char* v_lds = smem + SKV_MAX * KPITCH;

  const int tid = threadIdx.x, lane = tid & 63, wave_all = tid >> 6, nwaves = (blockDim.x >> 6) / KS2;
  const int wave = wave_all % nwaves, kpar = wave_all / nwaves;   // query tile within the chunk, key-tile parity (KS2 = 2)
  const int li = lane & 31, lh = lane >> 5;
  int bx, b, h;
  attn_block_coords(bx, h, b);
  const int D = p.D;
  const int kvlen = p.kv_len ? min(p.kv_len[b], p.Skv) : p.Skv;
  const char* kbase = p.k + ((int64_t)b * p.k_bs + (int64_t)h * D) * 2;
  const char* vbase = p.v + ((int64_t)b * p.v_bs + (int64_t)h * D) * 2;
  // heavy (late, causal) chunks first: the chunk index counts down
  const int chunk = (int)gridDim.x - 1 - bx;
  const int qt = chunk * nwaves + wave;                 // this wave's query tile
  const bool q_live = qt * 32 < p.Sq;
  const int qrow = qt * 32 + li;
  unsigned long long t_wait = 0;
  (void)t_wait;
  int kv_block_end = kvlen;                             // keys any wave of this block can see
  if (p.causal) kv_block_end = min(kv_block_end, (chunk + 1) * nwaves * 32);

  i32x4 qf[KS];
  {
    const char* qp = p.q + ((int64_t)b * p.q_bs + (int64_t)(qrow < p.Sq ? qrow : 0) * p.q_rs + (int64_t)h * D) * 2;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = ks * 16 + lh * 8;
      i32x4 z = {0, 0, 0, 0};
      qf[ks] = (qrow < p.Sq && d0 < D) ? *reinterpret_cast<const i32x4*>(qp + d0 * 2) : z;
    }
  }
  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.0f;
  float m_run = kNeg, l_run = 0.0f;

  for (int win0 = 0; win0 < kv_block_end; win0 += SKV_MAX) {
    const int win_keys = min(SKV_MAX, kv_block_end - win0);
    const int n_tiles = (win_keys + 31) >> 5;
    if (win0 > 0) __syncthreads();   // previous window fully consumed
    // ---- stage this window's K and V^T (rows >= Skv and dims >= D are zero) ------------------------------
    // kStageUn chunks per thread are requested before the first one is written: the staging pass pays ONE memory round trip per
    // group instead of one per chunk (ViT: 3456 chunks of K and of V over 576 threads = 6 per thread)
    constexpr int kStageUn = 3;
    const int n_chunks = n_tiles * 32 * CPR;
    for (int ch0 = tid; ch0 < n_chunks; ch0 += blockDim.x * kStageUn) {
      i32x4 kq[kStageUn], vq[kStageUn];
      int lrow_[kStageUn], cc_[kStageUn];
#pragma unroll
      for (int u = 0; u < kStageUn; ++u) {
        const int ch = ch0 + u * (int)blockDim.x;
        const int chc = ch < n_chunks ? ch : n_chunks - 1;
        const int t = chc / (32 * CPR), rem = chc - t * (32 * CPR);
        const int cc = rem >> 5, lrow = t * 32 + (rem & 31);
        const int row = win0 + lrow;
        const bool ok = (ch < n_chunks) && (row < p.Skv) && (cc * 8 < D);
        const i32x4 z = {0, 0, 0, 0};
        kq[u] = ok ? *reinterpret_cast<const i32x4*>(kbase + ((int64_t)row * p.k_rs + cc * 8) * 2) : z;
        vq[u] = ok ? *reinterpret_cast<const i32x4*>(vbase + ((int64_t)row * p.v_rs + cc * 8) * 2) : z;
        lrow_[u] = lrow;
        cc_[u] = cc;
      }
#pragma unroll
      for (int u = 0; u < kStageUn; ++u) {
        if (ch0 + u * (int)blockDim.x >= n_chunks) break;
        const int lrow = lrow_[u], cc = cc_[u];
        *reinterpret_cast<i32x4*>(k_lds + lrow * KPITCH + cc * 16) = kq[u];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t w = (uint32_t)vq[u][e];
          *reinterpret_cast<uint16_t*>(v_lds + (cc * 8 + 2 * e) * VPITCH + lrow * 2) = (uint16_t)(w & 0xffff);
          *reinterpret_cast<uint16_t*>(v_lds + (cc * 8 + 2 * e + 1) * VPITCH + lrow * 2) = (uint16_t)(w >> 16);
        }
      }
    }
    __syncthreads();
    if (!q_live) continue;
    {
    int t_end = n_tiles;
    if (p.causal) t_end = min(n_tiles, qt + 1 - (win0 >> 5));   // tiles up to this wave's diagonal
    for (int t = 0; t < t_end; ++t) {
      if (KS2 > 1 && (((win0 >> 5) + t) & (KS2 - 1)) != kpar) continue;   // the partner wave takes this key tile
      const int kv0 = win0 + t * 32;   // global key index of the tile; LDS rows are window-relative
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const i32x4 kf = *reinterpret_cast<const i32x4*>(k_lds + (t * 32 + li) * KPITCH + (ks * 2 + lh) * 16);
        s = Elem<T>::mfma(kf, qf[ks], s);
      }
      const bool need_mask = (kv0 + 32 > kvlen) || (p.causal && kv0 + 31 > qt * 32);
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const bool dead = (kv >= kvlen) || (p.causal && kv > qrow);
          s[r] = dead ? kNeg : s[r];
        }
      }
      float mx = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float mc = m_new * p.scale_log2;
      float rs = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(s[r], p.scale_log2, -mc));
        s[r] = pv;
        rs += pv;
      }
      rs += __shfl_xor(rs, 32, 64);
      if (__any(m_new != m_run)) {
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < DB; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
        m_run = m_new;
      }
      l_run += rs;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        i32x4 pf;
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[e] = (int)(Elem<T>::pack2(s[a * 8 + 2 * e], s[a * 8 + 2 * e + 1]));
#pragma unroll
        for (int i = 0; i < DB; ++i) {
          const char* vp = v_lds + (i * 32 + li) * VPITCH + (t * 32 + 16 * a + 4 * lh) * 2;
          const i32x2 lo = *reinterpret_cast<const i32x2*>(vp);
          const i32x2 hi = *reinterpret_cast<const i32x2*>(vp + 16);
          const i32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
          o[i] = Elem<T>::mfma(vf, pf, o[i]);
        }
      }
    }
    }
  }
  if constexpr (KS2 > 1) {
    // merge the two key-parity partials of every query tile: parity 1 parks (m, l, O) in LDS (the K/V windows are dead),
    // parity 0 combines:  m = max(m0, m1);  O = O0 * 2^((m0-m)*c) + O1 * 2^((m1-m)*c);  l likewise
    float* mbuf = reinterpret_cast<float*>(smem);
    for (int pp = 1; pp < KS2; ++pp) {   // one partner at a time: the merge buffer has to fit the (dead) K/V windows
      __syncthreads();
      if (kpar == pp) {
#pragma unroll
        for (int i = 0; i < DB; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) mbuf[((wave * (DB * 16 + 2) + i * 16 + r) << 6) + lane] = o[i][r];
        mbuf[((wave * (DB * 16 + 2) + DB * 16) << 6) + lane] = m_run;
        mbuf[((wave * (DB * 16 + 2) + DB * 16 + 1) << 6) + lane] = l_run;
      }
      __syncthreads();
      if (kpar == 0) {
        const float m1 = mbuf[((wave * (DB * 16 + 2) + DB * 16) << 6) + lane];
        const float l1 = mbuf[((wave * (DB * 16 + 2) + DB * 16 + 1) << 6) + lane];
        const float m = fmaxf(m_run, m1);
        const float a0 = __builtin_amdgcn_exp2f((m_run - m) * p.scale_log2), a1 = __builtin_amdgcn_exp2f((m1 - m) * p.scale_log2);
        l_run = l_run * a0 + l1 * a1;
        m_run = m;
#pragma unroll
        for (int i = 0; i < DB; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[i][r] = o[i][r] * a0 + mbuf[((wave * (DB * 16 + 2) + i * 16 + r) << 6) + lane] * a1;
      }
    }
    if (kpar != 0) return;
  }
  if (q_live && qrow < p.Sq) {
    const float inv = 1.0f / l_run;
    uint16_t* op = reinterpret_cast<uint16_t*>(p.o) + (int64_t)b * p.o_bs + (int64_t)qrow * p.o_rs + (int64_t)h * D;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = i * 32 + 8 * g + 4 * lh;
        if (d0 < D) {
          uint2 pk;
          pk.x = Elem<T>::pack2(o[i][4 * g + 0] * inv, o[i][4 * g + 1] * inv);
          pk.y = Elem<T>::pack2(o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv);
          *reinterpret_cast<uint2*>(op + d0) = pk;
        }
      }
    }
  }
}

// stllm_last_kernel() after stllm_attention: the kernel family and every parameter its dispatcher chose (the offset / ragged / segment entries name their own)
template <typename T> constexpr const char* attn_tname();
template <> constexpr const char* attn_tname<bf16_t>() { return "bf16_t"; }
template <> constexpr const char* attn_tname<f16_t>() { return "f16_t"; }
// One per launcher instantiation and thread (static thread_local): the name is formatted when the run-time parameters (key) change, a launch
// otherwise pays one compare; the string stays valid until the thread's next launch through the same instantiation.
struct AttnName {
  char s[96];
  int key = -1;
  template <typename... A> const char* get(int k, const char* fmt, A... a) {
    if (k != key) {
      snprintf(s, sizeof(s), fmt, a...);
      key = k;
    }
    return s;
  }
};

template <typename T, int DP, int SKV_MAX, int KS2 = 1>
int launch_resident(const AttnParams& p, hipStream_t stream, int nw_req = 0) {
  constexpr int lds = SKV_MAX * (DP * 2 + 16) + DP * (SKV_MAX * 2 + 8);

  static StllmPerDevice attr_dev;   // the dynamic-LDS opt-in is a per-device attribute
  bool attr_first;
  const int attr_d = attr_dev.enter(&attr_first);
  if (attr_first) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_resident_kernel<T, DP, SKV_MAX, KS2>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr_dev.done(attr_d);
  }
  const int q_tiles = (p.Sq + 31) / 32;
  int nw = nw_req > 0 ? nw_req : q_tiles;
  if (nw > 12) nw = 12;
  if (nw > q_tiles) nw = q_tiles;
  if (KS2 > 1 && nw * (DP / 32 * 16 + 2) * 256 > lds) {   // merge buffer (one parked (m, l, O) state per query tile) reuses the K/V windows
    stllm_set_error("stllm_attention: key-split merge buffer does not fit (nw=%d)", nw);
    return STLLM_ERR_UNSUPPORTED;
  }
  dim3 grid((q_tiles + nw - 1) / nw, p.H, p.B), block(64 * nw * KS2);
  static thread_local AttnName name;
  if (KS2 > 1) stllm_set_last_kernel(name.get(nw, "attn_resident_kernel<%s,%d,%d,%d> nw=%d", attn_tname<T>(), DP, SKV_MAX, KS2, nw));
  else stllm_set_last_kernel(name.get(0, "attn_resident_kernel<%s,%d,%d>", attn_tname<T>(), DP, SKV_MAX));
  hipLaunchKernelGGL((attn_resident_kernel<T, DP, SKV_MAX, KS2>), grid, block, lds, stream, p);
  STLLM_CHECK_LAUNCH("stllm_attention(resident)");
  return STLLM_OK;
}

// ---- D = 128 prefill (Llama), round 2: windows staged by LDS-DMA, V read through the hardware transpose ----------------------------
// Same work split as attn_resident_kernel<T, 128, 128, 4> (nw query tiles per workgroup, KS2 waves per query tile taking every
// KS2-th 32-key tile, 128-key windows, LDS merge at the end), but the staging no longer passes through registers:
//   * K and V rows of a window go global -> LDS with global_load_lds_dwordx4 (1 KiB = 4 rows per instruction, asynchronous) into
//     ROW-MAJOR images; window w + 1 is requested right after the barrier that starts window w and lands during its MFMAs:
//     ONE barrier per window, no ds_write, no V^T scatter (the old pass: 24 ds_write_b16 per thread and window);
//   * bank conflicts are avoided on the SOURCE side: LDS slot (row, 16-byte chunk c) holds logical chunk c ^ (row & 15) for K
//     (ds_read_b128 of 16 consecutive rows -> 16 different chunks) and c ^ ((row & 7) << 1) for V;
//   * V^T fragments come from ds_read_b64_tr_b16: in a 16-lane group lane i fetches 8 bytes of row (key) base + i / 4 at column
//     piece i % 4 and RECEIVES the four keys base .. base + 3 of column 4 (i / 4) + i % 4 = i — measured with tools/tr_probe.hip.
// two transposing reads, at p and p + OFF bytes (8 rows of the image further down); see the layout note above
template <int OFF = 2048>
__device__ __forceinline__ void lds_read_tr_pair(const char* p, unsigned long long& lo, unsigned long long& hi) {
  const unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(lo), "=&v"(hi) : "v"(a), "n"(OFF) : "memory");
}

// three pairs (d-blocks 0, 1, 2 of an UNSWIZZLED row: 64 bytes apart) with a single wait
template <int OFF>
__device__ __forceinline__ void lds_read_tr_3pairs(const char* p, unsigned long long& l0, unsigned long long& h0, unsigned long long& l1,
                                                   unsigned long long& h1, unsigned long long& l2, unsigned long long& h2) {
  const unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
  asm volatile("ds_read_b64_tr_b16 %0, %6\n\tds_read_b64_tr_b16 %1, %6 offset:%7\n\t"
               "ds_read_b64_tr_b16 %2, %6 offset:64\n\tds_read_b64_tr_b16 %3, %6 offset:%8\n\t"
               "ds_read_b64_tr_b16 %4, %6 offset:128\n\tds_read_b64_tr_b16 %5, %6 offset:%9\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1), "=&v"(l2), "=&v"(h2) : "v"(a), "n"(OFF), "n"(OFF + 64), "n"(OFF + 128) : "memory");
}

// NT: the launch's thread bound.  768 (12 waves: 3 per SIMD) caps the kernel at 168 registers and costs it 2-3 spilled ones; the prefill's 2 x 4 split
// (8 waves) is instantiated with 512: 256 registers, no scratch (round 6)
// four pairs at four addresses (the d-blocks of a SWIZZLED 256-byte row), ONE wait: eight reads in flight instead of four serialised round trips per 16-key step
template <int OFF>
__device__ __forceinline__ void lds_read_tr_4pairs(const char* p0, const char* p1, const char* p2, const char* p3, unsigned long long (&lo)[4], unsigned long long (&hi)[4]) {
  typedef __attribute__((address_space(3))) const char* lp;
  const unsigned a0 = (unsigned)(uintptr_t)(lp)p0, a1 = (unsigned)(uintptr_t)(lp)p1, a2 = (unsigned)(uintptr_t)(lp)p2, a3 = (unsigned)(uintptr_t)(lp)p3;
  asm volatile("ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %8 offset:%12\n\t"
               "ds_read_b64_tr_b16 %2, %9\n\tds_read_b64_tr_b16 %3, %9 offset:%12\n\t"
               "ds_read_b64_tr_b16 %4, %10\n\tds_read_b64_tr_b16 %5, %10 offset:%12\n\t"
               "ds_read_b64_tr_b16 %6, %11\n\tds_read_b64_tr_b16 %7, %11 offset:%12\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(lo[0]), "=&v"(hi[0]), "=&v"(lo[1]), "=&v"(hi[1]), "=&v"(lo[2]), "=&v"(hi[2]), "=&v"(lo[3]), "=&v"(hi[3])
               : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "n"(OFF) : "memory");
}

template <typename T, int KS2, int DP = 128, int NT = 768>
__global__ __launch_bounds__(NT) void attn_dma_kernel(const AttnParams p) {
  ATTN_STAMP(0);
  // DP = 128: Llama (256-byte rows, 128-key windows); DP = 96: head_dim 88 of the EVA ViT (rows of 11 chunks in a 12-chunk = 192-byte
  // pitch, chunk 11 a copy of chunk 10 that meets zero-padded Q / unstored columns; 96-key windows, two workgroups per CU)
  constexpr int KS = DP / 16, DB = DP / 32, CH = DP / 8, PITCH = CH * 16, W = DP == 128 ? 128 : 96;
  constexpr int kPieces = W * CH / 64;              // 1-KiB DMA pieces per image (32 / 18)
  constexpr int kImg = W * PITCH;                   // one K or V window image
  constexpr int kBuf = 2 * kImg;                   // [K | V]
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, nwv = blockDim.x >> 6, nwaves = nwv / KS2;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = wave_all % nwaves, kpar = wave_all / nwaves;
  const int li = lane & 31, lh = lane >> 5;
  int bx, b, h;
  attn_block_coords(bx, h, b);
  const int kvlen = p.kv_len ? min(p.kv_len[b], p.Skv) : p.Skv;
  const int D = p.D;
  const char* kbase = p.k + ((int64_t)b * p.k_bs + (int64_t)h * D) * 2;
  const char* vbase = p.v + ((int64_t)b * p.v_bs + (int64_t)h * D) * 2;
  auto swk = [](int row) { return DP == 128 ? (row & 15) : ((row >> 2) & 3); };          // K: 16-byte chunk XOR (bank spread of ds_read_b128 over 16 rows)
  auto swv = [](int row) { return DP == 128 ? ((row & 7) << 1) : 0; };                    // V: for the transposing reads (192-byte pitch needs none)
  const int chunk = (int)gridDim.x - 1 - bx;   // heavy (late, causal) chunks first
  const int qt = chunk * nwaves + wave;
  const bool q_live = qt * 32 < p.Sq;
  const int qrow = qt * 32 + li;
  unsigned long long t_wait = 0;
  (void)t_wait;
  int kv_block_end = kvlen;
  if (p.causal) kv_block_end = min(kv_block_end, (chunk + 1) * nwaves * 32);

  // The query fragments.  Straight from global memory every load instruction touches 32 rows = 32 cache lines for 32 bytes each, and the KS2 waves
  // of a tile fetch the same fragments: 8 x 32 line look-ups per wave at ~4.75 cycles each sat in FRONT of the first K / V window in the CU's
  // memory pipeline (timeline, tools/attn_trace.py: 7.7 k cycles from the start of a wave to its last request, profiles/r06_attn_trace.md).
  // p.q_lds: the tile's 32 rows arrive ONCE, row-contiguous, by LDS-DMA (CH / 2 one-KiB pieces shared by the tile's KS2 waves, K's chunk swizzle)
  // in an image behind the window buffers and are read as fragments after the first barrier.
  i32x4 qf[KS];
  if (!p.q_lds) {
    const char* qp = p.q + ((int64_t)b * p.q_bs + (int64_t)(qrow < p.Sq ? qrow : 0) * p.q_rs + (int64_t)h * D) * 2;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = ks * 16 + lh * 8;
      i32x4 z = {0, 0, 0, 0};
      qf[ks] = (qrow < p.Sq && d0 < D) ? *reinterpret_cast<const i32x4*>(qp + d0 * 2) : z;
    }
  }
  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.0f;
  float m_run = kNeg, l_run = 0.0f;
  char* qimg = smem + 2 * kBuf + wave * (32 * PITCH);
  if (p.q_lds) {
    const char* qb = p.q + ((int64_t)b * p.q_bs + (int64_t)h * D) * 2;
    const int lastc = (D * 2 + 15) / 16 - 1;
    for (int pc = kpar; pc < CH / 2; pc += KS2) {
      const int idx = pc * 64 + lane;
      const int r = idx / CH, pch = idx - r * CH;
      int lc = pch ^ swk(r);
      lc = lc < lastc ? lc : lastc;
      int row = qt * 32 + r;
      row = row < p.Sq ? row : p.Sq - 1;                            // rows past the end: a valid row, never stored
      glds16(qb + (int64_t)row * p.q_rs * 2 + lc * 16, qimg + (idx - lane) * 16);
    }
  }

  // ---- window DMA: 2 x kPieces pieces of 1 KiB per window (K image, then V image); piece pc is issued by wave pc % nwv -------------
  const int last_chunk = (D * 2 + 15) / 16 - 1;
  auto issue_window = [&](int win0, int buf) {
    for (int pc = wave_all; pc < 2 * kPieces; pc += nwv) {
      const bool is_v = pc >= kPieces;
      const int idx = (is_v ? pc - kPieces : pc) * 64 + lane;      // physical 16-byte slot of the image
      const int r4 = idx / CH, pch = idx - r4 * CH;                // window-relative row, physical chunk
      int lc = pch ^ (is_v ? swv(r4) : swk(r4));
      lc = lc < last_chunk ? lc : last_chunk;
      int row = win0 + r4;
      row = row < p.Skv ? row : p.Skv - 1;                         // rows past the end: a valid row (masked keys / zero weights)
      const char* src = (is_v ? vbase + (int64_t)row * p.v_rs * 2 : kbase + (int64_t)row * p.k_rs * 2) + lc * 16;
      glds16(src, smem + buf * kBuf + (is_v ? kImg : 0) + (idx - lane) * 16);
    }
  };
  const int n_win = (kv_block_end + W - 1) / W;
  if (n_win > 0) issue_window(0, 0);
  ATTN_STAMP(1);
  for (int w = 0; w < n_win; ++w) {
    const int win0 = w * W;
    const int n_tiles = (min(W, kv_block_end - win0) + 31) >> 5;
#ifdef STLLM_ATTN_TRACE
    const unsigned long long tw0 = __builtin_amdgcn_s_memtime();
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // my pieces of window w landed ...
    __syncthreads();                                    // ... everybody's did, and everybody is done with window w - 1
#ifdef STLLM_ATTN_TRACE
    t_wait += __builtin_amdgcn_s_memtime() - tw0;
    if (w == 0) ATTN_STAMP(2);
#endif
    if (w + 1 < n_win) issue_window(win0 + W, (w + 1) & 1);
    if (p.q_lds && w == 0) {   // (every piece of the tile landed before the barrier above: each wave drained its own queue first)
      const char* qa = qimg + li * PITCH;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const i32x4 z = {0, 0, 0, 0};
        const i32x4 f = *reinterpret_cast<const i32x4*>(qa + (((ks * 2 + lh) ^ swk(li)) << 4));
        qf[ks] = (ks * 16 + lh * 8 < D) ? f : z;                      // dims past D: K's chunk there is a copy of the last real one
      }
    }
    if (q_live) {
      const char* kimg = smem + (w & 1) * kBuf;
      const char* vimg = kimg + kImg;
      int t_end = n_tiles;
      if (p.causal) t_end = min(n_tiles, qt + 1 - (win0 >> 5));
      for (int t = 0; t < t_end; ++t) {
        if (KS2 > 1 && (((win0 >> 5) + t) & (KS2 - 1)) != kpar) continue;
        const int kv0 = win0 + t * 32;
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
        {
          const int row = t * 32 + li;
          const char* ka = kimg + row * PITCH;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const i32x4 kf = *reinterpret_cast<const i32x4*>(ka + (((ks * 2 + lh) ^ swk(row)) << 4));
            s = Elem<T>::mfma(kf, qf[ks], s);
          }
        }
        const bool need_mask = (kv0 + 32 > kvlen) || (p.causal && kv0 + 31 > qt * 32);
        if (need_mask) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv = kv0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const bool dead = (kv >= kvlen) || (p.causal && kv > qrow);
            s[r] = dead ? kNeg : s[r];
          }
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float mc = m_new * p.scale_log2;
        float rs = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = __builtin_amdgcn_exp2f(fmaf(s[r], p.scale_log2, -mc));
          s[r] = pv;
          rs += pv;
        }
        rs += __shfl_xor(rs, 32, 64);
        if (__any(m_new != m_run)) {
          const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);
          l_run *= alpha;
#pragma unroll
          for (int i = 0; i < DB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
          m_run = m_new;
        }
        l_run += rs;
        // P V: lane (d = li, lh) needs the keys 16 a + 4 lh + {0..3, 8..11} of column d: two transposing reads of four keys each
        const int i16 = lane & 15, jrow = i16 >> 2, piece = i16 & 3, cb = (li >> 4) * 4;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          i32x4 pf;
#pragma unroll
          for (int e = 0; e < 4; ++e) pf[e] = (int)(Elem<T>::pack2(s[a * 8 + 2 * e], s[a * 8 + 2 * e + 1]));
          if constexpr (NT == 512 && DB == 4) {
            // 256 registers (the 8-wave instantiation): the eight transposing reads of a 16-key step in flight together, one wait (under the 768-thread
            // bound's 168 registers the same block spilled and measured slower: 24.8 vs 22.7 us, round 2)
            const int row = t * 32 + 16 * a + 4 * lh + jrow;
            const char* rp = vimg + row * PITCH;
            auto ad = [&](int i) { const int pc8 = i * 8 + cb + piece; return rp + (((pc8 >> 1) ^ swv(row)) << 4) + ((pc8 & 1) << 3); };
            unsigned long long lo[4], hi[4];
            lds_read_tr_4pairs<8 * PITCH>(ad(0), ad(1), ad(2), ad(3), lo, hi);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const i32x4 vf = {(int)(unsigned)lo[i], (int)(unsigned)(lo[i] >> 32), (int)(unsigned)hi[i], (int)(unsigned)(hi[i] >> 32)};
              o[i] = Elem<T>::mfma(vf, pf, o[i]);
            }
          } else {
#pragma unroll
          for (int i = 0; i < DB; ++i) {
            unsigned long long lo, hi;
            {
              const int row = t * 32 + 16 * a + 4 * lh + jrow;       // (+ 8 for the second read: same row & 7)
              const int pc8 = i * 8 + cb + piece;                    // 8-byte piece of the row: column 32 i + 16 (li >> 4) + 4 piece
              lds_read_tr_pair<8 * PITCH>(vimg + row * PITCH + (((pc8 >> 1) ^ swv(row)) << 4) + ((pc8 & 1) << 3), lo, hi);
            }
            const i32x4 vf = {(int)(unsigned)lo, (int)(unsigned)(lo >> 32), (int)(unsigned)hi, (int)(unsigned)(hi >> 32)};
            o[i] = Elem<T>::mfma(vf, pf, o[i]);
          }
          }
        }
      }
    }
  }
  ATTN_STAMP(3);
  ATTN_STAMP_VAL(6, n_win);
  ATTN_STAMP_VAL(7, t_wait);
  if constexpr (KS2 > 1) {
    // merge of the KS2 partial (m, l, O) states of a query tile.  p.merge_par (launch_dma: (KS2 - 1) x nwaves parked states fit in the LDS): every
    // partner parks its state in its OWN slot, ONE barrier pair, the tile's first wave folds them in the fixed order 1, 2, .. (bit-identical to the
    // sequential rounds below, which cost two barriers per partner: 5.4 k cycles at KS2 = 4 in the timeline, profiles/r06_attn_trace.md)
    float* mbuf = reinterpret_cast<float*>(smem);
    constexpr int kState = DB * 16 + 2;
    auto fold = [&](int slot) {
      const float m1 = mbuf[((slot * kState + DB * 16) << 6) + lane];
      const float l1 = mbuf[((slot * kState + DB * 16 + 1) << 6) + lane];
      const float m = fmaxf(m_run, m1);
      const float a0 = __builtin_amdgcn_exp2f((m_run - m) * p.scale_log2), a1 = __builtin_amdgcn_exp2f((m1 - m) * p.scale_log2);
      l_run = l_run * a0 + l1 * a1;
      m_run = m;
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = o[i][r] * a0 + mbuf[((slot * kState + i * 16 + r) << 6) + lane] * a1;
    };
    auto park = [&](int slot) {
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) mbuf[((slot * kState + i * 16 + r) << 6) + lane] = o[i][r];
      mbuf[((slot * kState + DB * 16) << 6) + lane] = m_run;
      mbuf[((slot * kState + DB * 16 + 1) << 6) + lane] = l_run;
    };
    if (p.merge_par) {
      __syncthreads();
      if (kpar > 0) park((kpar - 1) * nwaves + wave);
      __syncthreads();
      if (kpar == 0)
        for (int pp = 1; pp < KS2; ++pp) fold((pp - 1) * nwaves + wave);
    } else {
      for (int pp = 1; pp < KS2; ++pp) {
        __syncthreads();
        if (kpar == pp) park(wave);
        __syncthreads();
        if (kpar == 0) fold(wave);
      }
    }
    ATTN_STAMP(4);
    if (kpar != 0) return;
  }
  if (q_live && qrow < p.Sq) {
    const float inv = 1.0f / l_run;
    uint16_t* op = reinterpret_cast<uint16_t*>(p.o) + (int64_t)b * p.o_bs + (int64_t)qrow * p.o_rs + (int64_t)h * D;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = i * 32 + 8 * g + 4 * lh;
        if (d0 < D) {
          uint2 pk;
          pk.x = Elem<T>::pack2(o[i][4 * g + 0] * inv, o[i][4 * g + 1] * inv);
          pk.y = Elem<T>::pack2(o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv);
          *reinterpret_cast<uint2*>(op + d0) = pk;
        }
      }
    }
  }
  ATTN_STAMP(5);
}

// ---- D = 88 (EVA ViT: 257 keys, padded to 96 dims x 288 keys): the same staging for the resident-K/V kernel -------------------------
// One workgroup per (frame, head) and query chunk, one wave per 32-row query tile, the whole K and V of the head in LDS as
// ROW-MAJOR images of 288 rows x 12 chunks of 16 bytes (chunk 11 = dims 88..95: a copy of chunk 10 — finite values that meet the
// zero-padded Q / unstored output columns).  The 108 KiB arrive by LDS-DMA in three windows of 96 keys (4 one-KiB pieces per wave
// and window at 9 waves); the waves start on window 0 while windows 1 and 2 are still in flight (counted vmcnt + one barrier per
// window).  K slot (row, c) holds logical chunk c ^ ((row >> 2) & 3) (rows are 48 dwords apart: rows r and r + 4 share banks);
// V needs no swizzle for the transposing reads (four consecutive rows = four disjoint 16-bank spans).
template <typename T>
__global__ __launch_bounds__(768) void attn_dma88_kernel(const AttnParams p) {
  ATTN_STAMP(0);
  constexpr int DP = 96, KS = DP / 16, DB = DP / 32, PITCH = 192, ROWS = 288;
  constexpr int kImg = ROWS * PITCH;                 // 55 296 bytes = 54 pieces of 1 KiB
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, nwaves = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  int bx, b, h;
  attn_block_coords(bx, h, b);
  const int D = p.D;
  const int kvlen = p.kv_len ? min(p.kv_len[b], p.Skv) : p.Skv;
  const char* kbase = p.k + ((int64_t)b * p.k_bs + (int64_t)h * D) * 2;
  const char* vbase = p.v + ((int64_t)b * p.v_bs + (int64_t)h * D) * 2;
  const int qt = bx * nwaves + wave;
  const bool q_live = qt * 32 < p.Sq;
  const int qrow = qt * 32 + li;

  // ---- staging: window w = rows 96 w .. 96 w + 95 of K (18 pieces) and of V (18 pieces); piece pc of a window by wave pc % nwaves
  auto issue_window = [&](int w) {
    for (int pc = wave; pc < 36; pc += nwaves) {
      const bool is_v = pc >= 18;
      const int idx = (w * 18 + (is_v ? pc - 18 : pc)) * 64 + lane;   // physical 16-byte slot of the image
      const int r = idx / 12, pch = idx - r * 12;
      int lc = is_v ? pch : (pch ^ ((r >> 2) & 3));
      lc = lc < 11 ? lc : 10;
      const int row = r < p.Skv ? r : p.Skv - 1;
      const char* src = (is_v ? vbase + (int64_t)row * p.v_rs * 2 : kbase + (int64_t)row * p.k_rs * 2) + lc * 16;
      glds16(src, smem + (is_v ? kImg : 0) + (idx - lane) * 16);
    }
  };
  i32x4 qf[KS];
  {
    const char* qp = p.q + ((int64_t)b * p.q_bs + (int64_t)(qrow < p.Sq ? qrow : 0) * p.q_rs + (int64_t)h * D) * 2;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = ks * 16 + lh * 8;
      i32x4 z = {0, 0, 0, 0};
      qf[ks] = (qrow < p.Sq && d0 < D) ? *reinterpret_cast<const i32x4*>(qp + d0 * 2) : z;
    }
  }
  asm volatile("" ::: "memory");   // the Q loads are OLDER than the window DMAs: the first counted wait below covers them
  const int n_win = (min(kvlen, ROWS) + 95) / 96;
  for (int w = 0; w < n_win; ++w) issue_window(w);
  ATTN_STAMP(1);
  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.0f;
  float m_run = kNeg, l_run = 0.0f;
  const char* kimg = smem;
  const char* vimg = smem + kImg;
  const int i16 = lane & 15, jrow = i16 >> 2, piece = i16 & 3, cb = (li >> 4) * 4;
  const int n_tiles = (min(kvlen, ROWS) + 31) >> 5;

  for (int w = 0; w < n_win; ++w) {
    // my pieces of windows 0..w landed (pieces are issued window by window, the same number per window for a given wave) ...
    // (counted only in the ViT's shape — 9 waves: exactly 4 pieces per wave and window; any other wave count drains everything)
    const int later = n_win - 1 - w;
    if (nwaves == 9 && later == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (nwaves == 9 && later == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                    // ... and everybody else's
    ATTN_STAMP(2 + 2 * (w < 2 ? w : 2));
    if (!q_live) continue;
    const int t_hi = min(n_tiles, 3 * (w + 1));
    for (int t = 3 * w; t < t_hi; ++t) {
      const int kv0 = t * 32;
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.0f;
      {
        const int row = t * 32 + li;
        const char* ka = kimg + row * PITCH;
        const int sw = (row >> 2) & 3;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const i32x4 kf = *reinterpret_cast<const i32x4*>(ka + (((ks * 2 + lh) ^ sw) << 4));
          s = Elem<T>::mfma(kf, qf[ks], s);
        }
      }
      if (kv0 + 32 > kvlen) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          s[r] = kv >= kvlen ? kNeg : s[r];
        }
      }
      float mx = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float mc = m_new * p.scale_log2;
      float rs = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(s[r], p.scale_log2, -mc));
        s[r] = pv;
        rs += pv;
      }
      rs += __shfl_xor(rs, 32, 64);
      if (__any(m_new != m_run)) {
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < DB; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
        m_run = m_new;
      }
      l_run += rs;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        i32x4 pf;
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[e] = (int)(Elem<T>::pack2(s[a * 8 + 2 * e], s[a * 8 + 2 * e + 1]));
        // the three pairs of transposing reads of this 16-key step in one block, ONE wait (registers to spare here: 120 of 170)
        unsigned long long l0, h0, l1, h1, l2, h2;
        {
          const int row = t * 32 + 16 * a + 4 * lh + jrow;
          lds_read_tr_3pairs<8 * PITCH>(vimg + row * PITCH + (cb + piece) * 8, l0, h0, l1, h1, l2, h2);
        }
        {
          const i32x4 v0 = {(int)(unsigned)l0, (int)(unsigned)(l0 >> 32), (int)(unsigned)h0, (int)(unsigned)(h0 >> 32)};
          const i32x4 v1 = {(int)(unsigned)l1, (int)(unsigned)(l1 >> 32), (int)(unsigned)h1, (int)(unsigned)(h1 >> 32)};
          const i32x4 v2 = {(int)(unsigned)l2, (int)(unsigned)(l2 >> 32), (int)(unsigned)h2, (int)(unsigned)(h2 >> 32)};
          o[0] = Elem<T>::mfma(v0, pf, o[0]);
          o[1] = Elem<T>::mfma(v1, pf, o[1]);
          o[2] = Elem<T>::mfma(v2, pf, o[2]);
        }
      }
    }
    ATTN_STAMP(3 + 2 * (w < 2 ? w : 2));
  }
  if (q_live && qrow < p.Sq) {
    const float inv = 1.0f / l_run;
    uint16_t* op = reinterpret_cast<uint16_t*>(p.o) + (int64_t)b * p.o_bs + (int64_t)qrow * p.o_rs + (int64_t)h * D;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = i * 32 + 8 * g + 4 * lh;
        if (d0 < D) {
          uint2 pk;
          pk.x = Elem<T>::pack2(o[i][4 * g + 0] * inv, o[i][4 * g + 1] * inv);
          pk.y = Elem<T>::pack2(o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv);
          *reinterpret_cast<uint2*>(op + d0) = pk;
        }
      }
    }
  }
}

template <typename T>
int launch_dma88(const AttnParams& p, hipStream_t stream) {
  constexpr int lds = 2 * 288 * 192;
  static StllmPerDevice attr_dev;   // the dynamic-LDS opt-in is a per-device attribute
  bool attr_first;
  const int attr_d = attr_dev.enter(&attr_first);
  if (attr_first) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_dma88_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr_dev.done(attr_d);
  }
  const int q_tiles = (p.Sq + 31) / 32;
  const int nw = q_tiles < 12 ? q_tiles : 12;
  dim3 grid((q_tiles + nw - 1) / nw, p.H, p.B), block(64 * nw);
  static thread_local AttnName name;
  stllm_set_last_kernel(name.get(0, "attn_dma88_kernel<%s>", attn_tname<T>()));
  hipLaunchKernelGGL((attn_dma88_kernel<T>), grid, block, lds, stream, p);
  STLLM_CHECK_LAUNCH("stllm_attention(dma88)");
  return STLLM_OK;
}

// env STLLM_ATTN_DMA / option "attn_dma" (stllm_options().attn_dma): 1 (default) LDS-DMA kernels for head_dim 128 (Llama prefill) and 88 (ViT) |
                              // 0 register-staged kernels everywhere
template <typename T, int KS2, int DP = 128, int NT = 768>
int launch_dma_nt(const AttnParams& p, hipStream_t stream, int nw_req) {
  constexpr int W = DP == 128 ? 128 : 96;
  constexpr int lds_win = 2 * 2 * W * (DP * 2);   // two buffers of [K | V] windows (128 KiB at 128 dims, 72 KiB at 96: two workgroups per CU)
  constexpr int lds_max = DP == 128 ? 160 * 1024 : 80 * 1024;
  static StllmPerDevice attr_dev;   // the dynamic-LDS opt-in is a per-device attribute
  bool attr_first;
  const int attr_d = attr_dev.enter(&attr_first);
  if (attr_first) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_dma_kernel<T, KS2, DP, NT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    attr_dev.done(attr_d);
  }
  const int q_tiles = (p.Sq + 31) / 32;
  int nw = nw_req < q_tiles ? nw_req : q_tiles;
  if (KS2 > 1 && nw * (DP / 32 * 16 + 2) * 256 > lds_win) {
    stllm_set_error("stllm_attention(dma): key-split merge buffer does not fit (nw=%d)", nw);
    return STLLM_ERR_UNSUPPORTED;
  }
  // query tiles through the LDS (attn_dma_kernel) when their images fit behind the window buffers; option attn_q_lds = 0: never (A/B)
  AttnParams pp = p;
  const int q_img = nw * 32 * (DP * 2);
  pp.q_lds = (stllm_options().attn_q_lds != 0 && lds_win + q_img <= lds_max && ((int64_t)p.q_rs * 2) % 16 == 0 && (p.D * 2) % 16 == 0) ? 1 : 0;
  const int lds = lds_win + (pp.q_lds ? q_img : 0);
  pp.merge_par = (KS2 > 1 && stllm_options().attn_q_lds != 0 && (KS2 - 1) * nw * (DP / 32 * 16 + 2) * 256 <= lds) ? 1 : 0;
  dim3 grid((q_tiles + nw - 1) / nw, p.H, p.B), block(64 * nw * KS2);
  static thread_local AttnName name;
  stllm_set_last_kernel(name.get(nw | pp.q_lds << 8 | pp.merge_par << 9, "attn_dma_kernel<%s,%d,%d,%d> nw=%d q_lds=%d merge_par=%d", attn_tname<T>(), KS2, DP, NT, nw, pp.q_lds,
                                 pp.merge_par));
  hipLaunchKernelGGL((attn_dma_kernel<T, KS2, DP, NT>), grid, block, lds, stream, pp);
  STLLM_CHECK_LAUNCH("stllm_attention(dma)");
  return STLLM_OK;
}

template <typename T, int KS2, int DP = 128>
int launch_dma(const AttnParams& p, hipStream_t stream, int nw_req) {
  const int q_tiles = (p.Sq + 31) / 32;
  const int nw = nw_req < q_tiles ? nw_req : q_tiles;
  if (64 * nw * KS2 <= 512 && stllm_options().attn_q_lds != 0) return launch_dma_nt<T, KS2, DP, 512>(p, stream, nw_req);
  return launch_dma_nt<T, KS2, DP, 768>(p, stream, nw_req);
}

// ---- exact fp32 path: one wave per query row -----------------------------------------------------
constexpr int kF32MaxKv = 2048;

// RAGGED (attn_f32_ragged_kernel, stllm_attention_offset_ragged): offset and length per batch row; a pad row is written as zeros and reads no key.
// SEG (attn_f32_segments_kernel, stllm_attention_segments): a segment of a packed buffer; a pad row does not exist, so it is neither read nor written.
template <bool RAGGED, bool SEG = false>
__device__ __forceinline__ void attn_f32_body(const typename AttnParamsOf<RAGGED, SEG>::type& p) {
  __shared__ float q_s[4][128];
  __shared__ float sc[4][kF32MaxKv];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qrow = blockIdx.x * 4 + w;
  if (qrow >= p.Sq) return;  // no block-level sync below
  const int D = p.D;
  const auto rr = [&] { if constexpr (SEG) return seg_row(p, b); else return ragged_row(p, b); }();
  const int kvlen = rr.kvlen;
  if constexpr (SEG) {
    if (qrow >= rr.n) return;
  }
  if constexpr (RAGGED && !SEG) {
    if (qrow >= rr.n) {
      float* o = reinterpret_cast<float*>(p.o) + (int64_t)b * p.o_bs + (int64_t)qrow * p.o_rs + (int64_t)h * p.D;
      for (int d = lane; d < p.D; d += 64) o[d] = 0.0f;
      return;
    }
  }
  const int kv_end = p.causal ? min(kvlen, (RAGGED ? rr.q_off : p.q_off) + qrow + 1) : kvlen;
  const float* q = reinterpret_cast<const float*>(p.q) + attn_q_base(p, rr, b) + (int64_t)qrow * p.q_rs + (int64_t)h * D;
  const float* kb = reinterpret_cast<const float*>(p.k) + (int64_t)attn_kv_row(p, rr, b) * p.k_bs + (int64_t)h * D;
  const float* vb = reinterpret_cast<const float*>(p.v) + (int64_t)attn_kv_row(p, rr, b) * p.v_bs + (int64_t)h * D;
  for (int d = lane; d < D; d += 64) q_s[w][d] = q[d];
  __builtin_amdgcn_wave_barrier();
  float mx = kNeg;
  for (int j = lane; j < kv_end; j += 64) {
    const float4* kr = reinterpret_cast<const float4*>(kb + (int64_t)j * p.k_rs);
    float acc = 0.0f;
    for (int d4 = 0; d4 < (D >> 2); ++d4) {
      const float4 kk = kr[d4];
      acc = fmaf(q_s[w][4 * d4 + 0], kk.x, acc);
      acc = fmaf(q_s[w][4 * d4 + 1], kk.y, acc);
      acc = fmaf(q_s[w][4 * d4 + 2], kk.z, acc);
      acc = fmaf(q_s[w][4 * d4 + 3], kk.w, acc);
    }
    acc *= p.scale;
    sc[w][j] = acc;
    mx = fmaxf(mx, acc);
  }
  mx = wave_max(mx);
  float sum = 0.0f;
  for (int j = lane; j < kv_end; j += 64) {
    const float e = expf(sc[w][j] - mx);
    sc[w][j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  __builtin_amdgcn_wave_barrier();
  const float inv = 1.0f / sum;
  float* o = reinterpret_cast<float*>(p.o) + attn_o_base(p, rr, b) + (int64_t)qrow * p.o_rs + (int64_t)h * D;
  for (int d = lane; d < D; d += 64) {
    float acc = 0.0f;
    for (int j = 0; j < kv_end; ++j) acc = fmaf(sc[w][j], vb[(int64_t)j * p.v_rs + d], acc);
    o[d] = acc * inv;
  }
}

__global__ __launch_bounds__(256) void attn_f32_kernel(const AttnParams p) { attn_f32_body<false>(p); }
__global__ __launch_bounds__(256) void attn_f32_ragged_kernel(const AttnRaggedParams p) { attn_f32_body<true>(p); }
__global__ __launch_bounds__(256) void attn_f32_segments_kernel(const AttnSegParams p) { attn_f32_body<true, true>(p); }

// ---- exact fp32 path on the MATRIX cores (round 4): v_mfma_f32_32x32x2_f32, bit-equal to an fmaf chain per output --------------------
// The one-wave-per-row kernel above re-reads the whole K and V of a head from L2 for every query row (181 KB per ViT row: ~12 GB per
// layer) and ran at 3.6 % of the fp32 vector peak: 58 of the 117 ms of a split-verify step (profiles/r04_split_step.md).  This kernel is
// attn_mfma_kernel's schedule in fp32: a wave owns 32 query rows, 32-key tiles of K (row-major) and V^T go through LDS once per
// WORKGROUP (register-staged one tile ahead), S^T = K Q^T and O^T += V^T P^T are chains of 32x32x2 fp32 MFMAs (K = 2 per instruction:
// DP / 2 + 16 DP / 32 of them per tile), softmax statistics per lane exactly as in the 16-bit kernels.  A 16-byte LDS read feeds four MFMAs
// (the k <-> (step, half) slot map only has to agree between the A and the B operand, Elem<float>::mfma).
template <int DP, int NW>
__global__ __launch_bounds__(64 * NW) void attn_mfma_f32_kernel(const AttnParams p) {
  constexpr int KS8 = DP / 8;           // 16-byte K fragments per row half-pair: lane half lh holds d = 8 ks + 4 lh .. + 3
  constexpr int DB = DP / 32;           // 32-row blocks of O^T
  constexpr int KPITCH = DP * 4 + 16;   // bytes per K row in LDS
  constexpr int VPITCH = 32 * 4 + 16;   // bytes per V^T row (32 keys) in LDS
  constexpr int NT = 64 * NW;
  constexpr int CPR = DP / 4;           // 16-byte chunks per K / V row
  constexpr int NCH = 32 * CPR;
  constexpr int CPT = (NCH + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) char k_lds[32 * KPITCH];
  __shared__ __attribute__((aligned(16))) char v_lds[DP * VPITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q_blk0 = blockIdx.x * (32 * NW);
  const int qrow = q_blk0 + wave * 32 + li;
  const int D = p.D;
  const int kvlen = p.kv_len ? min(p.kv_len[b], p.Skv) : p.Skv;

  f32x4 qf[KS8];   // B operand of S^T: Q[q = li][8 ks + 4 lh .. + 3]
  {
    const float* qp = reinterpret_cast<const float*>(p.q) + (int64_t)b * p.q_bs + (int64_t)(qrow < p.Sq ? qrow : 0) * p.q_rs + (int64_t)h * D;
#pragma unroll
    for (int ks = 0; ks < KS8; ++ks) {
      const int d0 = ks * 8 + lh * 4;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      qf[ks] = (qrow < p.Sq && d0 < D) ? *reinterpret_cast<const f32x4*>(qp + d0) : z;   // D % 4 == 0
    }
  }
  f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.0f;
  float m_run = kNeg, l_run = 0.0f;

  int kv_end = kvlen;
  if (p.causal) kv_end = min(kv_end, p.q_off + q_blk0 + 32 * NW);
  const float* kbase = reinterpret_cast<const float*>(p.k) + (int64_t)b * p.k_bs + (int64_t)h * D;
  const float* vbase = reinterpret_cast<const float*>(p.v) + (int64_t)b * p.v_bs + (int64_t)h * D;
  f32x4 kreg[CPT], vreg[CPT];
  auto load_tile = [&](int kv0) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int ch = tid + c * NT;
      const int cc = ch >> 5, row = ch & 31;   // consecutive lanes = consecutive keys: conflict-free transposed V writes
      const int kv = kv0 + row;
      const bool ok = (ch < NCH) && (kv < p.Skv) && (cc * 4 < D);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      kreg[c] = ok ? *reinterpret_cast<const f32x4*>(kbase + (int64_t)kv * p.k_rs + cc * 4) : z;
      vreg[c] = ok ? *reinterpret_cast<const f32x4*>(vbase + (int64_t)kv * p.v_rs + cc * 4) : z;
    }
  };
  const int wave_q_last = p.q_off + q_blk0 + wave * 32 + 31;
  if (kv_end > 0) load_tile(0);
  for (int kv0 = 0; kv0 < kv_end; kv0 += 32) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int ch = tid + c * NT;
      if (ch < NCH) {
        const int cc = ch >> 5, row = ch & 31;
        *reinterpret_cast<f32x4*>(k_lds + row * KPITCH + cc * 16) = kreg[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) *reinterpret_cast<float*>(v_lds + (cc * 4 + e) * VPITCH + row * 4) = vreg[c][e];
      }
    }
    __syncthreads();
    if (kv0 + 32 < kv_end) load_tile(kv0 + 32);
    if (p.causal && kv0 > wave_q_last) continue;

    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS8; ++ks) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(k_lds + li * KPITCH + (ks * 2 + lh) * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[ks][e], s, 0, 0, 0);
    }
    const bool need_mask = (kv0 + 32 > kvlen) || (p.causal && kv0 + 31 > p.q_off + q_blk0 + wave * 32);
    if (need_mask) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv = kv0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const bool dead = (kv >= kvlen) || (p.causal && kv > qrow + p.q_off);
        s[r] = dead ? kNeg : s[r];
      }
    }
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float mc = m_new * p.scale_log2;
    float rs = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pv = exp2f(fmaf(s[r], p.scale_log2, -mc));   // the library exp2f (full fp32 accuracy), not the hardware approximation
      s[r] = pv;
      rs += pv;
    }
    rs += __shfl_xor(rs, 32, 64);
    if (__any(m_new != m_run)) {
      const float alpha = exp2f((m_run - m_new) * p.scale_log2);
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
      m_run = m_new;
    }
    l_run += rs;
    // O^T[d][q] += V^T[d][kv] P^T[kv][q]: the lane's score register r is key (r & 3) + 8 (r >> 2) + 4 lh — registers 4 g .. 4 g + 3 are four
    // consecutive keys 8 g + 4 lh ..: one 16-byte read of the V^T row feeds their four MFMAs
#pragma unroll
    for (int i = 0; i < DB; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 vf = *reinterpret_cast<const f32x4*>(v_lds + (i * 32 + li) * VPITCH + (8 * g + 4 * lh) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[e], s[4 * g + e], o[i], 0, 0, 0);
      }
    }
  }
  if (qrow < p.Sq) {
    const float inv = 1.0f / l_run;
    float* op = reinterpret_cast<float*>(p.o) + (int64_t)b * p.o_bs + (int64_t)qrow * p.o_rs + (int64_t)h * D;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = i * 32 + 8 * g + 4 * lh;
        if (d0 < D) {
          const f32x4 ov = {o[i][4 * g + 0] * inv, o[i][4 * g + 1] * inv, o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv};
          *reinterpret_cast<f32x4*>(op + d0) = ov;
        }
      }
    }
  }
}

template <int DP, int NW>
int launch_mfma_f32(const AttnParams& p, hipStream_t stream, bool named = false) {
  dim3 grid((p.Sq + 32 * NW - 1) / (32 * NW), p.H, p.B), block(64 * NW);
  static thread_local AttnName name;
  if (named) stllm_set_last_kernel(name.get(0, "attn_mfma_f32_kernel<%d,%d>", DP, NW));
  hipLaunchKernelGGL((attn_mfma_f32_kernel<DP, NW>), grid, block, 0, stream, p);
  STLLM_CHECK_LAUNCH("stllm_attention(fp32 mfma)");
  return STLLM_OK;
}

// fp32: matrix-core kernel from 8 query rows on (prefill shapes), the vector kernel for the one-row decode step and tiny problems.
// named: stllm_attention's call — the launch names itself (stllm_attention_offset has set its own, shorter name before it comes here)
int dispatch_f32(const AttnParams& p, hipStream_t stream, int mode, bool named = false) {
  if (mode != 0 && p.Sq >= 8) {
    const int nw = p.Sq <= 32 ? 1 : (p.Sq <= 64 ? 2 : 3);
    if (p.D == 64) return nw == 1 ? launch_mfma_f32<64, 1>(p, stream, named) : nw == 2 ? launch_mfma_f32<64, 2>(p, stream, named) : launch_mfma_f32<64, 3>(p, stream, named);
    if (p.D == 88) return nw == 1 ? launch_mfma_f32<96, 1>(p, stream, named) : nw == 2 ? launch_mfma_f32<96, 2>(p, stream, named) : launch_mfma_f32<96, 3>(p, stream, named);
    if (p.D == 128) return nw == 1 ? launch_mfma_f32<128, 1>(p, stream, named) : nw == 2 ? launch_mfma_f32<128, 2>(p, stream, named) : launch_mfma_f32<128, 3>(p, stream, named);
  }
  if (p.Skv > kF32MaxKv) {
    stllm_set_error("stllm_attention(fp32, vector kernel): Skv %d > %d", p.Skv, kF32MaxKv);
    return STLLM_ERR_BAD_SHAPE;
  }
  dim3 grid((p.Sq + 3) / 4, p.H, p.B), block(256);
  if (named) stllm_set_last_kernel("attn_f32_kernel");
  hipLaunchKernelGGL(attn_f32_kernel, grid, block, 0, stream, p);
  STLLM_CHECK_LAUNCH("stllm_attention(fp32)");
  return STLLM_OK;
}

template <typename T, int DP, int NW>
int launch_mfma(const AttnParams& p, hipStream_t stream, bool named = false) {   // named: as in dispatch_f32
  dim3 grid((p.Sq + 32 * NW - 1) / (32 * NW), p.H, p.B), block(64 * NW);
  static thread_local AttnName name;
  if (named) stllm_set_last_kernel(name.get(0, "attn_mfma_kernel<%s,%d,%d>", attn_tname<T>(), DP, NW));
  hipLaunchKernelGGL((attn_mfma_kernel<T, DP, NW>), grid, block, 0, stream, p);
  STLLM_CHECK_LAUNCH("stllm_attention");
  return STLLM_OK;
}

template <typename T>
int dispatch(const AttnParams& p, hipStream_t stream) {
  // NW picked so that 32*NW divides the common sequence lengths with little waste:
  //   ViT 257 -> 3 waves (96 rows, 3 blocks), Q-Former 32/44 -> 1-2 waves, Llama -> 3 waves (576 = 6*96)
  if (p.D == 88) {
    if (p.Sq <= 32) return launch_mfma<T, 96, 1>(p, stream, true);                 // BT-Adapter temporal attention
    if (p.Skv <= 288 && !p.causal) {
      const int g_attn_dma = stllm_options().attn_dma;
      const bool al = ((reinterpret_cast<uintptr_t>(p.k) | reinterpret_cast<uintptr_t>(p.v)) & 15) == 0 && (p.k_rs % 8) == 0 && (p.v_rs % 8) == 0 &&
                      (p.k_bs % 8) == 0 && (p.v_bs % 8) == 0;
      // LDS-DMA staging in three 96-key windows + transposing V reads: 23.2 vs 24.1 us for the register-staged resident kernel (both
      // after the XCD-aware block mapping; 26.3 vs 27.1 before it)
      if (g_attn_dma != 0 && al) return launch_dma88<T>(p, stream);
      return launch_resident<T, 96, 288>(p, stream);
    }  // ViT: K/V of a head resident in LDS (a key split here re-stages K/V per query chunk: 26 -> 37 us)
    return launch_mfma<T, 96, 3>(p, stream, true);
  }
  if (p.D == 64) return p.Sq <= 32 ? launch_mfma<T, 64, 1>(p, stream, true) : launch_mfma<T, 64, 2>(p, stream, true);
  if (p.D == 128) {
    const int g_attn_dma = stllm_options().attn_dma;
    const bool al = ((reinterpret_cast<uintptr_t>(p.k) | reinterpret_cast<uintptr_t>(p.v)) & 15) == 0 && (p.k_rs % 8) == 0 && (p.v_rs % 8) == 0 &&
                    (p.k_bs % 8) == 0 && (p.v_bs % 8) == 0;
    if (g_attn_dma != 0 && al && p.Skv >= 1) {   // LDS-DMA windows + transposing V reads (round 2)
      // query tiles per workgroup x waves per query tile, measured at S = 576, 32 heads (us at B = 1 / B = 4): 12 x 1: 27.1 / 33.0,
      // 6 x 2: 27.1 / 48.6, 4 x 2: 21.5 / 53.4, 3 x 4: 22.7 / 62.1 (register-staged kernel: 28.0 / 75.3) — the fewest key-split
      // waves that still give >= 128 workgroups
      const int q_tiles = (p.Sq + 31) / 32, bh = p.B * p.H;
      if (g_attn_dma >= 10) {   // experiments (tools/attn_bench.py --audit): attn_dma = 10 x (query tiles per workgroup) + (waves per query tile), at most 12 waves
        const int nwf = g_attn_dma / 10, ks = g_attn_dma % 10;
        if (nwf >= 1 && nwf * ks <= 12) {
          if (ks == 1) return launch_dma<T, 1>(p, stream, nwf);
          if (ks == 2) return launch_dma<T, 2>(p, stream, nwf);
          if (ks == 4) return launch_dma<T, 4>(p, stream, nwf);
        }
      }
      // round 4 (tools/attn_bench.py --audit, profiles/r04_attn_dispatch_audit.log): one sequence of <= 640 positions (32 heads) runs best as 2 query tiles x 4 key-split
      // waves per workgroup — 10.8 / 13.0 / 14.9 / 19.0 / 19.1 us at S = 178 / 296 / 400 / 528 / 576 against 14.2 / 16.2 / 17.0 / 20.5 / 20.6 on the rules below
      if (bh <= 32 && q_tiles <= 20) return launch_dma<T, 4>(p, stream, 2);
      if (bh * ((q_tiles + 11) / 12) >= 128) return launch_dma<T, 1>(p, stream, 12);
      if (bh * ((q_tiles + 3) / 4) >= 128) return launch_dma<T, 2>(p, stream, 4);
      return launch_dma<T, 4>(p, stream, 3);
    }
    return launch_resident<T, 128, 128, 4>(p, stream, 3);
  }   // + four waves per query tile (every 4th key tile each)  // 128-key windows (2 workgroups/CU), 96 queries per workgroup
  stllm_set_error("stllm_attention: unsupported head_dim %d", p.D);
  return STLLM_ERR_UNSUPPORTED;
}

}  // namespace

// =====================================================================================================
// Decode attention (Sq = 1 against a KV cache): HBM-bound streaming of K and V.
// The tile kernels above give one query tile per head = 32 workgroups walking the cache serially (38 us per layer
// at Skv = 580).  Here the keys are split across `nsplit` workgroups per (batch, head):
//   partial kernel: 4 waves per workgroup, wave w takes keys k0 + w, k0 + w + 4, ...; lane l owns dims 2l, 2l+1
//     (one 4-byte load per lane = one coalesced 256-byte row per wave), score = butterfly-reduced dot, online softmax
//     in the exp2 domain, O accumulated in 2 registers per lane; the 4 waves merge through LDS and write (m, l, O[128]);
//   merge kernel: one workgroup per (batch, head) combines the nsplit partials and writes the output row.
// =====================================================================================================
constexpr int kDecD = 128;
constexpr int kDecRec = kDecD + 2;   // floats per partial record: m, l, O[128]

template <typename T> __device__ __forceinline__ void widen2(uint32_t u, float& a, float& b);
template <> __device__ __forceinline__ void widen2<bf16_t>(uint32_t u, float& a, float& b) {
  a = __builtin_bit_cast(float, u << 16);
  b = __builtin_bit_cast(float, u & 0xffff0000u);
}
template <> __device__ __forceinline__ void widen2<f16_t>(uint32_t u, float& a, float& b) {
  a = (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu));
  b = (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
}

// the body of one split-KV workgroup of the RAGGED kernel: keys [k0, k1) of (b, h), partial state -> its record (Skv, split count and keys per split are
// read per batch row by the caller).  The same key-to-lane assignment and merge order as attn_decode_partial_kernel below, so equal lengths give equal bits.
template <typename T>
__device__ __forceinline__ void decode_partial_body(const AttnParams& p, float (&part)[4][kDecRec], float* __restrict__ ws, int rec_stride, int sp, int b, int h, int k0, int k1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float q0, q1;
  widen2<T>(*reinterpret_cast<const uint32_t*>(p.q + ((int64_t)b * p.q_bs + (int64_t)h * kDecD + 2 * lane) * 2), q0, q1);
  q0 *= p.scale_log2;
  q1 *= p.scale_log2;
  const char* kb = p.k + ((int64_t)b * p.k_bs + (int64_t)h * kDecD + 2 * lane) * 2;
  const char* vb = p.v + ((int64_t)b * p.v_bs + (int64_t)h * kDecD + 2 * lane) * 2;
  float m = kNeg, l = 0.0f, o0 = 0.0f, o1 = 0.0f;
  for (int key = k0 + wave; key < k1; key += 4) {
    float ka, kc, va, vc;
    widen2<T>(*reinterpret_cast<const uint32_t*>(kb + (int64_t)key * p.k_rs * 2), ka, kc);
    widen2<T>(*reinterpret_cast<const uint32_t*>(vb + (int64_t)key * p.v_rs * 2), va, vc);
    const float s = wave_sum(fmaf(q0, ka, q1 * kc));   // log2-domain score, identical in every lane
    const float mn = fmaxf(m, s);
    const float alpha = __builtin_amdgcn_exp2f(m - mn), pr = __builtin_amdgcn_exp2f(s - mn);
    l = fmaf(l, alpha, pr);
    o0 = fmaf(o0, alpha, pr * va);
    o1 = fmaf(o1, alpha, pr * vc);
    m = mn;
  }
  if (lane == 0) { part[wave][0] = m; part[wave][1] = l; }
  part[wave][2 + 2 * lane] = o0;
  part[wave][3 + 2 * lane] = o1;
  __syncthreads();
  if (wave == 0) {
    float mm = fmaxf(fmaxf(part[0][0], part[1][0]), fmaxf(part[2][0], part[3][0]));
    float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = __builtin_amdgcn_exp2f(part[w][0] - mm);
      ll = fmaf(part[w][1], f, ll);
      a0 = fmaf(part[w][2 + 2 * lane], f, a0);
      a1 = fmaf(part[w][3 + 2 * lane], f, a1);
    }
    float* rec = ws + (((int64_t)b * p.H + h) * rec_stride + sp) * kDecRec;   // rec_stride: records per (batch, head) = the split count of the grid
    if (lane == 0) { rec[0] = mm; rec[1] = ll; }
    rec[2 + 2 * lane] = a0;
    rec[3 + 2 * lane] = a1;
  }
}

// The uniform split-KV workgroup keeps its own copy of the loop above, statement for statement: routed through decode_partial_body the compiler schedules it
// differently (profiles/ragged_decode_uniform_isa_diff.log), and the uniform path's instruction streams are not to change with the ragged feature.  The two
// copies must stay in step: tests/test_ragged_gpu.py::test_attention_decode_ragged compares them bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void attn_decode_partial_kernel(const AttnParams p, float* __restrict__ ws, int nsplit, int keys_per_split) {
  __shared__ float part[4][kDecRec];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int k0 = sp * keys_per_split, k1 = min(p.Skv, k0 + keys_per_split);
  float q0, q1;
  widen2<T>(*reinterpret_cast<const uint32_t*>(p.q + ((int64_t)b * p.q_bs + (int64_t)h * kDecD + 2 * lane) * 2), q0, q1);
  q0 *= p.scale_log2;
  q1 *= p.scale_log2;
  const char* kb = p.k + ((int64_t)b * p.k_bs + (int64_t)h * kDecD + 2 * lane) * 2;
  const char* vb = p.v + ((int64_t)b * p.v_bs + (int64_t)h * kDecD + 2 * lane) * 2;
  float m = kNeg, l = 0.0f, o0 = 0.0f, o1 = 0.0f;
  for (int key = k0 + wave; key < k1; key += 4) {
    float ka, kc, va, vc;
    widen2<T>(*reinterpret_cast<const uint32_t*>(kb + (int64_t)key * p.k_rs * 2), ka, kc);
    widen2<T>(*reinterpret_cast<const uint32_t*>(vb + (int64_t)key * p.v_rs * 2), va, vc);
    const float s = wave_sum(fmaf(q0, ka, q1 * kc));   // log2-domain score, identical in every lane
    const float mn = fmaxf(m, s);
    const float alpha = __builtin_amdgcn_exp2f(m - mn), pr = __builtin_amdgcn_exp2f(s - mn);
    l = fmaf(l, alpha, pr);
    o0 = fmaf(o0, alpha, pr * va);
    o1 = fmaf(o1, alpha, pr * vc);
    m = mn;
  }
  if (lane == 0) { part[wave][0] = m; part[wave][1] = l; }
  part[wave][2 + 2 * lane] = o0;
  part[wave][3 + 2 * lane] = o1;
  __syncthreads();
  if (wave == 0) {
    float mm = fmaxf(fmaxf(part[0][0], part[1][0]), fmaxf(part[2][0], part[3][0]));
    float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = __builtin_amdgcn_exp2f(part[w][0] - mm);
      ll = fmaf(part[w][1], f, ll);
      a0 = fmaf(part[w][2 + 2 * lane], f, a0);
      a1 = fmaf(part[w][3 + 2 * lane], f, a1);
    }
    float* rec = ws + (((int64_t)b * p.H + h) * nsplit + sp) * kDecRec;
    if (lane == 0) { rec[0] = mm; rec[1] = ll; }
    rec[2 + 2 * lane] = a0;
    rec[3 + 2 * lane] = a1;
  }
}

template <typename T>
__device__ __forceinline__ void decode_merge_body(const AttnParams& p, const float* __restrict__ ws, int rec_stride, int nsplit, int b, int h) {
  const int lane = threadIdx.x;
  const float* rec = ws + ((int64_t)b * p.H + h) * rec_stride * kDecRec;
  float mm = kNeg;
  for (int s = 0; s < nsplit; ++s) mm = fmaxf(mm, rec[s * kDecRec]);
  float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
  for (int s = 0; s < nsplit; ++s) {
    const float f = __builtin_amdgcn_exp2f(rec[s * kDecRec] - mm);
    ll = fmaf(rec[s * kDecRec + 1], f, ll);
    a0 = fmaf(rec[s * kDecRec + 2 + 2 * lane], f, a0);
    a1 = fmaf(rec[s * kDecRec + 3 + 2 * lane], f, a1);
  }
  const float inv = 1.0f / ll;
  uint32_t* op = reinterpret_cast<uint32_t*>(p.o + ((int64_t)b * p.o_bs + (int64_t)h * kDecD + 2 * lane) * 2);
  *op = Elem<T>::pack2(a0 * inv, a1 * inv);
}

template <typename T>
__global__ __launch_bounds__(64) void attn_decode_merge_kernel(const AttnParams p, const float* __restrict__ ws, int nsplit) {
  const int h = blockIdx.x, b = blockIdx.y;
  decode_merge_body<T>(p, ws, nsplit, nsplit, b, h);
}

// ---- single-pass decode attention (round 2): ONE workgroup of 16 waves per (batch, head) ---------------------------------------
// The split-KV pair above costs two launches (10.5 + 7.7 us per layer at Skv = 580) for 0.3 MB of K/V per head.  Here a wave works on
// FOUR keys at a time: 16 lanes per key, 8 dims = one 16-byte load per lane for K and for V (4x wider than the 4-byte loads above),
// a 4-step butterfly inside the 16-lane group, an online-softmax state per lane group; the next step's K/V are requested before the
// current step is consumed.  The 4 x 16 partial states of the workgroup are merged through LDS (8.3 KB).  Used when the cache is
// short enough that 16 waves per head cover it in a few steps (Skv <= kDecSingleMax) or when B * H alone fills the chip.
constexpr int kDecSingleMax = 1536;
constexpr int kDecWaves = 16;

template <typename T> __device__ __forceinline__ void widen8v(i32x4 v, float* f);
template <> __device__ __forceinline__ void widen8v<bf16_t>(i32x4 v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = __builtin_bit_cast(float, (uint32_t)v[e] << 16);
    f[2 * e + 1] = __builtin_bit_cast(float, (uint32_t)v[e] & 0xffff0000u);
  }
}
template <> __device__ __forceinline__ void widen8v<f16_t>(i32x4 v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t u = (uint32_t)v[e];
    f[2 * e] = (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu));
    f[2 * e + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
  }
}

// body shared by the uniform kernel (Skv = p.Skv) and the ragged one (Skv = the batch row's own length, workgroup-uniform)
template <typename T>
__device__ __forceinline__ void decode_single_body(const AttnParams& p, float (&part)[kDecWaves * 4][kDecRec], int b, int h, int Skv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane >> 4, l16 = lane & 15;     // key within the wave's quad, dims 8 * l16 .. + 7
  float q[8];
  widen8v<T>(*reinterpret_cast<const i32x4*>(p.q + ((int64_t)b * p.q_bs + (int64_t)h * kDecD + 8 * l16) * 2), q);
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] *= p.scale_log2;
  const char* kb = p.k + ((int64_t)b * p.k_bs + (int64_t)h * kDecD + 8 * l16) * 2;
  const char* vb = p.v + ((int64_t)b * p.v_bs + (int64_t)h * kDecD + 8 * l16) * 2;
  float m = kNeg, l = 0.0f, o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.0f;
  const int step = kDecWaves * 4;
  int kbase = wave * 4;                              // wave-uniform: all four lane groups run the same number of steps
  i32x4 kn = {0, 0, 0, 0}, vn = {0, 0, 0, 0};
  if (kbase + grp < Skv) {
    kn = *reinterpret_cast<const i32x4*>(kb + (int64_t)(kbase + grp) * p.k_rs * 2);
    vn = *reinterpret_cast<const i32x4*>(vb + (int64_t)(kbase + grp) * p.v_rs * 2);
  }
  for (; kbase < Skv; kbase += step) {
    const int key = kbase + grp;
    const bool live = key < Skv;
    const i32x4 kc = kn, vc = vn;
    const int nk = key + step;
    if (nk < Skv) {   // request the next quad of this wave before this one is consumed
      kn = *reinterpret_cast<const i32x4*>(kb + (int64_t)nk * p.k_rs * 2);
      vn = *reinterpret_cast<const i32x4*>(vb + (int64_t)nk * p.v_rs * 2);
    }
    float kf[8], vf[8];
    widen8v<T>(kc, kf);
    widen8v<T>(vc, vf);
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(q[e], kf[e], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);                       // log2-domain score of this group's key, identical in its 16 lanes
    if (live) {
      const float mn = fmaxf(m, s);
      const float alpha = __builtin_amdgcn_exp2f(m - mn), pr = __builtin_amdgcn_exp2f(s - mn);
      l = fmaf(l, alpha, pr);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf(o[e], alpha, pr * vf[e]);
      m = mn;
    }
  }
  float* rec = part[wave * 4 + grp];
  if (l16 == 0) { rec[0] = m; rec[1] = l; }
#pragma unroll
  for (int e = 0; e < 8; ++e) rec[2 + 8 * l16 + e] = o[e];
  __syncthreads();
  if (threadIdx.x < kDecD) {
    const int d = threadIdx.x;
    float mm = kNeg;
    for (int r = 0; r < kDecWaves * 4; ++r) mm = fmaxf(mm, part[r][0]);
    float ll = 0.0f, acc = 0.0f;
    for (int r = 0; r < kDecWaves * 4; ++r) {
      const float f = __builtin_amdgcn_exp2f(part[r][0] - mm);
      ll = fmaf(part[r][1], f, ll);
      acc = fmaf(part[r][2 + d], f, acc);
    }
    store_elem<T>(p.o, (int64_t)b * p.o_bs + (int64_t)h * kDecD + d, acc / ll);
  }
}

template <typename T>
__global__ __launch_bounds__(64 * kDecWaves) void attn_decode_single_kernel(const AttnParams p) {
  __shared__ float part[kDecWaves * 4][kDecRec];   // one (m, l, O[128]) record per 16-lane group
  decode_single_body<T>(p, part, blockIdx.y, blockIdx.x, p.Skv);
}

// stllm_set_option("attn_decode_single", 0): always the split-KV pair (tests compare both)
__host__ __device__ static inline int decode_splits(int Skv) {
  int n = (Skv + 47) / 48;   // ~48 keys (12 per wave) per workgroup
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}

// ---- ragged decode attention: every batch row has its own number of cached keys (kv_len[b], device memory; max_kv bounds it on the host) -------
// The bodies above with the length read once per workgroup.  Row b of the split pair uses the split count and keys per split that the uniform call
// gives Skv = kv_len[b] (decode_splits): the grid is sized for max_kv, surplus workgroups exit, the merge reads the records its row wrote — at the
// record stride of the grid (nsplit_max).  A row of length 0 (a free slot of the batch) writes zeros.
__device__ __forceinline__ void decode_zero_row(const AttnParams& p, int b, int h) {
  if (threadIdx.x < 64) *reinterpret_cast<uint32_t*>(p.o + ((int64_t)b * p.o_bs + (int64_t)h * kDecD + 2 * threadIdx.x) * 2) = 0u;
}

template <typename T>
__global__ __launch_bounds__(64 * kDecWaves) void attn_decode_single_ragged_kernel(const AttnParams p) {
  __shared__ float part[kDecWaves * 4][kDecRec];
  const int h = blockIdx.x, b = blockIdx.y;
  const int len = min(p.kv_len[b], p.Skv);
  if (len <= 0) { decode_zero_row(p, b, h); return; }
  decode_single_body<T>(p, part, b, h, len);
}

template <typename T>
__global__ __launch_bounds__(256) void attn_decode_partial_ragged_kernel(const AttnParams p, float* __restrict__ ws, int nsplit_max) {
  __shared__ float part[4][kDecRec];
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int len = min(p.kv_len[b], p.Skv);
  const int nsplit = decode_splits(len);
  if (len <= 0 || sp >= nsplit) return;
  const int kps = (len + nsplit - 1) / nsplit;
  const int k0 = sp * kps, k1 = min(len, k0 + kps);
  decode_partial_body<T>(p, part, ws, nsplit_max, sp, b, h, k0, k1);
}

template <typename T>
__global__ __launch_bounds__(64) void attn_decode_merge_ragged_kernel(const AttnParams p, const float* __restrict__ ws, int nsplit_max) {
  const int h = blockIdx.x, b = blockIdx.y;
  const int len = min(p.kv_len[b], p.Skv);
  if (len <= 0) { decode_zero_row(p, b, h); return; }
  decode_merge_body<T>(p, ws, nsplit_max, decode_splits(len), b, h);
}

extern "C" int stllm_attention(int dtype, const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs,
                               int64_t k_rs, const void* v, int64_t v_bs, int64_t v_rs, void* out, int64_t o_bs,
                               int64_t o_rs, int B, int H, int Sq, int Skv, int D, float scale, int causal,
                               const int32_t* kv_len, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(q && k && v && out, "stllm_attention: null pointer");
  STLLM_CHECK_ARG(B > 0 && H > 0 && Sq > 0 && Skv > 0, "stllm_attention: empty problem");
  STLLM_CHECK_ARG(D == 64 || D == 88 || D == 128, "stllm_attention: head_dim %d not in {64,88,128}", D);
  STLLM_CHECK_ARG(!causal || Sq == Skv, "stllm_attention: causal needs Sq == Skv");
  STLLM_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out), "stllm_attention: pointers must be 16-byte aligned");
  STLLM_CHECK_ARG(q_rs % 8 == 0 && k_rs % 8 == 0 && v_rs % 8 == 0 && o_rs % 8 == 0 && q_bs % 8 == 0 && k_bs % 8 == 0 &&
                      v_bs % 8 == 0 && o_bs % 8 == 0, "stllm_attention: strides must be multiples of 8 elements");
  AttnParams p{};
  p.q = (const char*)q; p.q_bs = q_bs; p.q_rs = q_rs;
  p.k = (const char*)k; p.k_bs = k_bs; p.k_rs = k_rs;
  p.v = (const char*)v; p.v_bs = v_bs; p.v_rs = v_rs;
  p.o = (char*)out; p.o_bs = o_bs; p.o_rs = o_rs;
  p.B = B; p.H = H; p.Sq = Sq; p.Skv = Skv; p.D = D;
  p.scale = scale; p.scale_log2 = scale * 1.44269504088896340736f;
  p.causal = causal; p.kv_len = kv_len;
  switch (dtype) {
    case STLLM_BF16: return dispatch<bf16_t>(p, stream);
    case STLLM_F16: return dispatch<f16_t>(p, stream);
    case STLLM_F32: return dispatch_f32(p, stream, stllm_options().attn_f32_mfma, true);
  }
  stllm_set_error("stllm_attention: bad dtype %d", dtype);
  return STLLM_ERR_BAD_DTYPE;
}


// =====================================================================================================
// Attention with a query offset (a suffix of Sq positions appended behind q_off cached ones: LlamaModel.extend).
//   tile path: attn_mfma_kernel / attn_mfma_f32_kernel / attn_f32_kernel with AttnParams.q_off in their causal predicates and tile bounds;
//   key-split path (16-bit, D = 128): few query tiles against many keys is 32 heads x 1-3 query tiles = a few dozen workgroups, each walking
//     every key tile serially.  The keys of one (batch, head, query chunk) are split into `nsplit` ranges of whole 32-key tiles; one workgroup
//     of attn_mfma_kernel<.., SPLIT> per range leaves (O, m, l) per query row in the workspace, attn_ksplit_merge_kernel combines the ranges in
//     ascending order (deterministic) and writes the compute-dtype rows.  Two launches, no flags, no polling.
// =====================================================================================================
namespace {

// RAGGED: a pad query row (every record of it is empty: 1 / ll would be infinite) is written as zeros.
// SEG: a pad row of a segment does not exist in the packed buffer: nothing is written for it.
template <typename T, bool RAGGED = false, bool SEG = false>
__global__ __launch_bounds__(64) void attn_ksplit_merge_kernel(const typename AttnParamsOf<RAGGED, SEG>::type p) {
  const int lane = threadIdx.x, qrow = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  if constexpr (SEG) {
    if (qrow >= seg_row(p, b).n) return;
  }
  if constexpr (RAGGED && !SEG) {
    if (qrow >= ragged_row(p, b).n) {
      *reinterpret_cast<uint32_t*>(p.o + ((int64_t)b * p.o_bs + (int64_t)qrow * p.o_rs + (int64_t)h * 128 + 2 * lane) * 2) = 0u;
      return;
    }
  }
  const float* rec = p.ws + (((int64_t)b * p.H + h) * p.Sq + qrow) * p.nsplit * kSplRec;
  float mm = kNeg;
  for (int s = 0; s < p.nsplit; ++s) mm = fmaxf(mm, rec[s * kSplRec + 128]);
  float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
  for (int s = 0; s < p.nsplit; ++s) {
    const float f = __builtin_amdgcn_exp2f((rec[s * kSplRec + 128] - mm) * p.scale_log2);   // empty ranges: exp2(-huge) == 0
    ll = fmaf(rec[s * kSplRec + 129], f, ll);
    a0 = fmaf(rec[s * kSplRec + 2 * lane], f, a0);
    a1 = fmaf(rec[s * kSplRec + 2 * lane + 1], f, a1);
  }
  const float inv = 1.0f / ll;
  uint32_t* op;
  if constexpr (SEG) op = reinterpret_cast<uint32_t*>(p.o + ((int64_t)(seg_row(p, b).row0 + qrow) * p.o_rs + (int64_t)h * 128 + 2 * lane) * 2);
  else op = reinterpret_cast<uint32_t*>(p.o + ((int64_t)b * p.o_bs + (int64_t)qrow * p.o_rs + (int64_t)h * 128 + 2 * lane) * 2);
  *op = Elem<T>::pack2(a0 * inv, a1 * inv);
}

// waves (= 32-row query tiles) per workgroup and key ranges per query chunk of the key-split path: a pure function of the shape, shared by the
// workspace query and the launch.  Ranges are whole 32-key tiles, at least two tiles each, at most 16 ranges; enough of them for ~512 workgroups.
struct KsplitPlan { int nw, chunks, nsplit, kps; };
KsplitPlan ksplit_plan(int B, int H, int Sq, int Skv) {
  KsplitPlan pl;
  const int q_tiles = (Sq + 31) / 32;
  pl.nw = q_tiles < 4 ? q_tiles : 4;
  pl.chunks = (q_tiles + pl.nw - 1) / pl.nw;
  const int tiles = (Skv + 31) / 32;
  const int64_t wgs = (int64_t)B * H * pl.chunks;
  int want = (int)((512 + wgs - 1) / wgs);
  if (want > 16) want = 16;
  if (want > tiles / 2) want = tiles / 2;
  if (want < 1) want = 1;
  const int tps = (tiles + want - 1) / want;
  pl.kps = tps * 32;
  pl.nsplit = (tiles + tps - 1) / tps;
  return pl;
}

template <typename T, int NW, bool RAGGED, bool SEG>
void launch_ksplit_nw(const typename AttnParamsOf<RAGGED, SEG>::type& p, const KsplitPlan& pl, hipStream_t stream) {
  hipLaunchKernelGGL((attn_mfma_kernel<T, 128, NW, true, RAGGED, RAGGED, SEG>), dim3(pl.chunks * pl.nsplit, p.H, p.B), dim3(64 * NW), 0, stream, p);
}

template <typename T, bool RAGGED = false, bool SEG = false>
int launch_ksplit(typename AttnParamsOf<RAGGED, SEG>::type p, hipStream_t stream) {
  const KsplitPlan pl = ksplit_plan(p.B, p.H, p.Sq, p.Skv);
  p.nsplit = pl.nsplit;
  p.kps = pl.kps;
  switch (pl.nw) {
    case 1: launch_ksplit_nw<T, 1, RAGGED, SEG>(p, pl, stream); break;
    case 2: launch_ksplit_nw<T, 2, RAGGED, SEG>(p, pl, stream); break;
    case 3: launch_ksplit_nw<T, 3, RAGGED, SEG>(p, pl, stream); break;
    default: launch_ksplit_nw<T, 4, RAGGED, SEG>(p, pl, stream); break;
  }
  hipLaunchKernelGGL((attn_ksplit_merge_kernel<T, RAGGED, SEG>), dim3(p.Sq, p.H, p.B), dim3(64), 0, stream, p);
  STLLM_CHECK_LAUNCH(SEG ? "stllm_attention_segments(key split)" : RAGGED ? "stllm_attention_offset_ragged(key split)" : "stllm_attention_offset(key split)");
  stllm_set_last_kernel("attn_ksplit_kernel");
  return STLLM_OK;
}

// the dispatch rule of the key-split path.  stllm_set_option("attn_ksplit", 1 / 0) forces it on (wherever it is eligible) / off.
// tools/attn_bench.py --suffix (MI355X, bf16, 32 heads, graph replays, us tile -> key split; profiles/prefix_cache.md): Sq = 8: 38 -> 14 / 69 -> 18 / 142 -> 26 at
// q_off = 512 / 1024 / 2048; Sq = 40: 38 -> 17 / 68 -> 23 / 137 -> 27 (q_off = 128: 15 -> 12, 256: 23 -> 13); Sq = 96: 40 -> 21 / 70 -> 31 / 142 -> 40;
// Sq = 200 behind 1024: 83 -> 34; Sq = 320 behind 2048: 155 -> 73; five beams' worth (B = 5, Sq = 40 behind 1024): 75 -> 52.  It won on every shape measured, so the
// rule is the measured region: up to 320 (batch, head, query tile) triples and at least 160 keys.  Larger problems fill the chip with query tiles alone and were
// not measured: they stay on the tile kernel.
bool ksplit_wins(const AttnParams& p) {
  const int q_tiles = (p.Sq + 31) / 32;
  return (int64_t)p.B * p.H * q_tiles <= 320 && p.Skv >= 160;
}

template <typename T>
int dispatch_offset(const AttnParams& p, hipStream_t stream) {
  const int opt = stllm_options().attn_ksplit;
  if (p.D == 128 && p.ws && opt != 0 && (opt > 0 || ksplit_wins(p))) return launch_ksplit<T>(p, stream);
  stllm_set_last_kernel("attn_mfma_kernel");
  const int nw = p.Sq <= 32 ? 1 : (p.Sq <= 64 ? 2 : 3);
  if (p.D == 128) return nw == 1 ? launch_mfma<T, 128, 1>(p, stream) : nw == 2 ? launch_mfma<T, 128, 2>(p, stream) : launch_mfma<T, 128, 3>(p, stream);
  if (p.D == 88) return nw == 1 ? launch_mfma<T, 96, 1>(p, stream) : launch_mfma<T, 96, 3>(p, stream);
  return nw == 1 ? launch_mfma<T, 64, 1>(p, stream) : launch_mfma<T, 64, 2>(p, stream);
}

template <typename T, int NW>
int launch_mfma_ragged(const AttnRaggedParams& p, hipStream_t stream) {
  dim3 grid((p.Sq + 32 * NW - 1) / (32 * NW), p.H, p.B), block(64 * NW);
  hipLaunchKernelGGL((attn_mfma_kernel<T, 128, NW, false, true, true>), grid, block, 0, stream, p);
  STLLM_CHECK_LAUNCH("stllm_attention_offset_ragged");
  return STLLM_OK;
}

// stllm_attention_offset_ragged, 16-bit at head_dim 128: dispatch_offset's two schedules — the same plan and the same waves per workgroup at (B, H, Sq, max_kv) —
// on the RAGGED instantiations.  The rule is the region measured on ragged rows (tools/attn_bench.py --ragged-suffix, MI355X, bf16, 32 heads, graph replays,
// us tile -> key split; profiles/ragged_extend.md): B = 4, prefixes 300 - 610, n = 8: 47 -> 22; prefixes 560 - 1100, n = 8 - 40: 77 -> 33; prefixes 330 - 1024 with
// one row at n = 0: 70 -> 30; prefixes 580 - 620, n = 20: 50 -> 24; B = 8, prefixes 300 - 1100, n = 8: 80 -> 52, n = 8 - 40 (two query tiles, 512 triples): 78 -> 50.
// It won on every shape measured, so: up to 512 (batch, head, query tile) triples — ksplit_wins stops at 320, where its own measurements end — and at least 160
// keys (below ~ 600 keys the bound is ksplit_wins', measured on uniform rows only).  Larger problems were not measured: they stay on the tile kernel.
bool ksplit_wins_ragged(const AttnParams& p) {
  const int q_tiles = (p.Sq + 31) / 32;
  return (int64_t)p.B * p.H * q_tiles <= 512 && p.Skv >= 160;
}

template <typename T>
int dispatch_offset_ragged(const AttnRaggedParams& p, hipStream_t stream) {
  const int opt = stllm_options().attn_ksplit;
  if (p.ws && opt != 0 && (opt > 0 || ksplit_wins_ragged(p))) return launch_ksplit<T, true>(p, stream);
  stllm_set_last_kernel("attn_mfma_kernel");
  const int nw = p.Sq <= 32 ? 1 : (p.Sq <= 64 ? 2 : 3);
  return nw == 1 ? launch_mfma_ragged<T, 1>(p, stream) : nw == 2 ? launch_mfma_ragged<T, 2>(p, stream) : launch_mfma_ragged<T, 3>(p, stream);
}

// stllm_attention_segments: dispatch_offset_ragged on the SEG instantiations — the same rule, plan and waves per workgroup at (R, H, max_n, max_kv).
template <typename T, int NW>
int launch_mfma_segments(const AttnSegParams& p, hipStream_t stream) {
  dim3 grid((p.Sq + 32 * NW - 1) / (32 * NW), p.H, p.B), block(64 * NW);
  hipLaunchKernelGGL((attn_mfma_kernel<T, 128, NW, false, true, true, true>), grid, block, 0, stream, p);
  STLLM_CHECK_LAUNCH("stllm_attention_segments");
  return STLLM_OK;
}

template <typename T>
int dispatch_segments(const AttnSegParams& p, hipStream_t stream) {
  const int opt = stllm_options().attn_ksplit;
  if (p.ws && opt != 0 && (opt > 0 || ksplit_wins_ragged(p))) return launch_ksplit<T, true, true>(p, stream);
  stllm_set_last_kernel("attn_mfma_kernel");
  const int nw = p.Sq <= 32 ? 1 : (p.Sq <= 64 ? 2 : 3);
  return nw == 1 ? launch_mfma_segments<T, 1>(p, stream) : nw == 2 ? launch_mfma_segments<T, 2>(p, stream) : launch_mfma_segments<T, 3>(p, stream);
}

}  // namespace

extern "C" int64_t stllm_attention_offset_workspace_bytes(int B, int H, int Sq, int Skv) {
  if (B <= 0 || H <= 0 || Sq <= 0 || Skv <= 0) return -1;
  return (int64_t)B * H * Sq * ksplit_plan(B, H, Sq, Skv).nsplit * kSplRec * 4;
}

extern "C" int stllm_attention_offset(int dtype, const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs,
                                      int64_t k_rs, const void* v, int64_t v_bs, int64_t v_rs, void* out, int64_t o_bs,
                                      int64_t o_rs, int B, int H, int Sq, int Skv, int D, float scale, int causal,
                                      const int32_t* kv_len, int q_off, void* workspace, int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(q && k && v && out, "stllm_attention_offset: null pointer");
  STLLM_CHECK_ARG(B > 0 && H > 0 && Sq > 0 && Skv > 0, "stllm_attention_offset: empty problem");
  STLLM_CHECK_ARG(D == 64 || D == 88 || D == 128, "stllm_attention_offset: head_dim %d not in {64,88,128}", D);
  STLLM_CHECK_ARG(q_off >= 0 && (int64_t)q_off + Sq <= Skv, "stllm_attention_offset: needs 0 <= q_off and q_off + Sq <= Skv (q_off %d, Sq %d, Skv %d)", q_off, Sq, Skv);
  STLLM_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out), "stllm_attention_offset: pointers must be 16-byte aligned");
  STLLM_CHECK_ARG(q_rs % 8 == 0 && k_rs % 8 == 0 && v_rs % 8 == 0 && o_rs % 8 == 0 && q_bs % 8 == 0 && k_bs % 8 == 0 &&
                      v_bs % 8 == 0 && o_bs % 8 == 0, "stllm_attention_offset: strides must be multiples of 8 elements");
  AttnParams p{};
  p.q = (const char*)q; p.q_bs = q_bs; p.q_rs = q_rs;
  p.k = (const char*)k; p.k_bs = k_bs; p.k_rs = k_rs;
  p.v = (const char*)v; p.v_bs = v_bs; p.v_rs = v_rs;
  p.o = (char*)out; p.o_bs = o_bs; p.o_rs = o_rs;
  p.B = B; p.H = H; p.Sq = Sq; p.Skv = Skv; p.D = D;
  p.scale = scale; p.scale_log2 = scale * 1.44269504088896340736f;
  p.causal = causal; p.kv_len = kv_len;
  p.q_off = causal ? q_off : 0;   // without the causal mask the offset has no effect
  // the key-split path needs its workspace; a call without one (or with too small a one) runs the tile kernels
  if (workspace && aligned16(workspace) && workspace_bytes >= stllm_attention_offset_workspace_bytes(B, H, Sq, Skv)) p.ws = reinterpret_cast<float*>(workspace);
  switch (dtype) {
    case STLLM_BF16: return dispatch_offset<bf16_t>(p, stream);
    case STLLM_F16: return dispatch_offset<f16_t>(p, stream);
    case STLLM_F32:
      // the vector kernel keeps a row's scores in LDS (Skv <= 2048) and is the one-row kernel: longer caches run the matrix-core kernel at any Sq
      if (Skv > kF32MaxKv && D == 128 && (Sq < 8 || stllm_options().attn_f32_mfma == 0)) {
        stllm_set_last_kernel("attn_mfma_f32_kernel");
        return launch_mfma_f32<128, 1>(p, stream);
      }
      stllm_set_last_kernel(stllm_options().attn_f32_mfma != 0 && Sq >= 8 ? "attn_mfma_f32_kernel" : "attn_f32_kernel");
      return dispatch_f32(p, stream, stllm_options().attn_f32_mfma);
  }
  stllm_set_error("stllm_attention_offset: bad dtype %d", dtype);
  return STLLM_ERR_BAD_DTYPE;
}

extern "C" int64_t stllm_attention_offset_ragged_workspace_bytes(int B, int H, int Sq, int max_kv) {
  return stllm_attention_offset_workspace_bytes(B, H, Sq, max_kv);
}

// stllm_attention_offset with a query offset and a length PER BATCH ROW (always causal): row b holds q_off[b] cached positions and kv_len[b] - q_off[b]
// (0 .. Sq) new ones.  Schedule, plan and grid come from (B, H, Sq, max_kv) exactly as stllm_attention_offset derives them from Skv; the per-row bounds
// live in the kernels (attn_mfma_kernel<.., LIVE, RAGGED>, attn_ksplit_merge_kernel<T, RAGGED>, attn_f32_ragged_kernel).
extern "C" int stllm_attention_offset_ragged(int dtype, const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs,
                                             int64_t k_rs, const void* v, int64_t v_bs, int64_t v_rs, void* out, int64_t o_bs,
                                             int64_t o_rs, int B, int H, int Sq, int max_kv, int D, float scale, const int32_t* q_off,
                                             const int32_t* kv_len, void* workspace, int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(q && k && v && out && q_off && kv_len, "stllm_attention_offset_ragged: null pointer");
  STLLM_CHECK_ARG(B > 0 && H > 0 && Sq > 0 && max_kv > 0, "stllm_attention_offset_ragged: empty problem");
  if (D != 128 || (dtype != STLLM_BF16 && dtype != STLLM_F16 && dtype != STLLM_F32)) {
    stllm_set_error("stllm_attention_offset_ragged: head_dim %d / dtype %d unsupported (bf16 / fp16 / fp32 at head_dim 128)", D, dtype);
    return STLLM_ERR_UNSUPPORTED;
  }
  if (dtype == STLLM_F32 && max_kv > kF32MaxKv) {
    stllm_set_error("stllm_attention_offset_ragged: fp32 with max_kv %d > %d unsupported (the vector kernel keeps a row's scores in the LDS)", max_kv, kF32MaxKv);
    return STLLM_ERR_UNSUPPORTED;
  }
  STLLM_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out), "stllm_attention_offset_ragged: pointers must be 16-byte aligned");
  STLLM_CHECK_ARG(q_rs % 8 == 0 && k_rs % 8 == 0 && v_rs % 8 == 0 && o_rs % 8 == 0 && q_bs % 8 == 0 && k_bs % 8 == 0 &&
                      v_bs % 8 == 0 && o_bs % 8 == 0, "stllm_attention_offset_ragged: strides must be multiples of 8 elements");
  STLLM_CHECK_ARG(((reinterpret_cast<uintptr_t>(q_off) | reinterpret_cast<uintptr_t>(kv_len)) & 3) == 0, "stllm_attention_offset_ragged: tables must be 4-byte aligned");
  AttnRaggedParams p{};
  p.q = (const char*)q; p.q_bs = q_bs; p.q_rs = q_rs;
  p.k = (const char*)k; p.k_bs = k_bs; p.k_rs = k_rs;
  p.v = (const char*)v; p.v_bs = v_bs; p.v_rs = v_rs;
  p.o = (char*)out; p.o_bs = o_bs; p.o_rs = o_rs;
  p.B = B; p.H = H; p.Sq = Sq; p.Skv = max_kv; p.D = D;
  p.scale = scale; p.scale_log2 = scale * 1.44269504088896340736f;
  p.causal = 1; p.kv_len = kv_len; p.q_off_tab = q_off;
  if (workspace && aligned16(workspace) && workspace_bytes >= stllm_attention_offset_ragged_workspace_bytes(B, H, Sq, max_kv)) p.ws = reinterpret_cast<float*>(workspace);
  if (dtype == STLLM_F32) {
    stllm_set_last_kernel("attn_f32_kernel");
    hipLaunchKernelGGL(attn_f32_ragged_kernel, dim3((Sq + 3) / 4, H, B), dim3(256), 0, stream, p);
    STLLM_CHECK_LAUNCH("stllm_attention_offset_ragged(fp32)");
    return STLLM_OK;
  }
  return dtype == STLLM_BF16 ? dispatch_offset_ragged<bf16_t>(p, stream) : dispatch_offset_ragged<f16_t>(p, stream);
}

extern "C" int64_t stllm_attention_segments_workspace_bytes(int R, int H, int max_n, int max_kv) {
  return stllm_attention_offset_workspace_bytes(R, H, max_n, max_kv);
}

// stllm_attention_offset_ragged on a PACKED query buffer: segment r = (slot[r], row0[r], q_off[r], kv_len[r]) reads the K / V of cache row slot[r] and owns the
// packed rows row0[r] .. row0[r] + n_r - 1 of q and out (n_r = kv_len[r] - q_off[r] after ragged_row's clamps, at most max_n).  Schedule, plan and grid come
// from (R, H, max_n, max_kv); the per-segment bounds and the table guard live in the kernels (seg_row).
extern "C" int stllm_attention_segments(int dtype, const void* q, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v, int64_t v_bs,
                                        int64_t v_rs, void* out, int64_t o_rs, int R, int H, int D, int T, int n_slots, int max_n, int max_kv, float scale,
                                        const int32_t* slot, const int32_t* row0, const int32_t* q_off, const int32_t* kv_len, void* workspace,
                                        int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(q && k && v && out && slot && row0 && q_off && kv_len, "stllm_attention_segments: null pointer");
  STLLM_CHECK_ARG(R > 0 && R <= 65535 && H > 0 && T > 0 && n_slots > 0 && max_n > 0 && max_kv > 0, "stllm_attention_segments: empty problem (or R > 65535)");
  if (D != 128 || (dtype != STLLM_BF16 && dtype != STLLM_F16 && dtype != STLLM_F32)) {
    stllm_set_error("stllm_attention_segments: head_dim %d / dtype %d unsupported (bf16 / fp16 / fp32 at head_dim 128)", D, dtype);
    return STLLM_ERR_UNSUPPORTED;
  }
  if (dtype == STLLM_F32 && max_kv > kF32MaxKv) {
    stllm_set_error("stllm_attention_segments: fp32 with max_kv %d > %d unsupported (the vector kernel keeps a row's scores in the LDS)", max_kv, kF32MaxKv);
    return STLLM_ERR_UNSUPPORTED;
  }
  STLLM_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out), "stllm_attention_segments: pointers must be 16-byte aligned");
  STLLM_CHECK_ARG(q_rs % 8 == 0 && k_rs % 8 == 0 && v_rs % 8 == 0 && o_rs % 8 == 0 && k_bs % 8 == 0 && v_bs % 8 == 0,
                  "stllm_attention_segments: strides must be multiples of 8 elements");
  STLLM_CHECK_ARG(((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(row0) | reinterpret_cast<uintptr_t>(q_off) |
                    reinterpret_cast<uintptr_t>(kv_len)) & 3) == 0, "stllm_attention_segments: tables must be 4-byte aligned");
  AttnSegParams p{};
  p.q = (const char*)q; p.q_bs = 0; p.q_rs = q_rs;
  p.k = (const char*)k; p.k_bs = k_bs; p.k_rs = k_rs;
  p.v = (const char*)v; p.v_bs = v_bs; p.v_rs = v_rs;
  p.o = (char*)out; p.o_bs = 0; p.o_rs = o_rs;
  p.B = R; p.H = H; p.Sq = max_n; p.Skv = max_kv; p.D = D;
  p.scale = scale; p.scale_log2 = scale * 1.44269504088896340736f;
  p.causal = 1; p.kv_len = kv_len; p.q_off_tab = q_off;
  p.slot = slot; p.row0 = row0; p.T = T; p.n_slots = n_slots;
  if (workspace && aligned16(workspace) && workspace_bytes >= stllm_attention_segments_workspace_bytes(R, H, max_n, max_kv)) p.ws = reinterpret_cast<float*>(workspace);
  if (dtype == STLLM_F32) {
    stllm_set_last_kernel("attn_f32_kernel");
    hipLaunchKernelGGL(attn_f32_segments_kernel, dim3((max_n + 3) / 4, H, R), dim3(256), 0, stream, p);
    STLLM_CHECK_LAUNCH("stllm_attention_segments(fp32)");
    return STLLM_OK;
  }
  return dtype == STLLM_BF16 ? dispatch_segments<bf16_t>(p, stream) : dispatch_segments<f16_t>(p, stream);
}

extern "C" int64_t stllm_attention_decode_workspace_bytes(int B, int H, int Skv) {
  if (B <= 0 || H <= 0 || Skv <= 0) return -1;
  return (int64_t)B * H * decode_splits(Skv) * kDecRec * 4;
}

extern "C" int stllm_attention_decode(int dtype, const void* q, int64_t q_bs, const void* k, int64_t k_bs, int64_t k_rs,
                                      const void* v, int64_t v_bs, int64_t v_rs, void* out, int64_t o_bs, int B, int H, int Skv,
                                      int D, float scale, void* workspace, int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(q && k && v && out && workspace, "stllm_attention_decode: null pointer");
  STLLM_CHECK_ARG(B > 0 && H > 0 && Skv > 0, "stllm_attention_decode: empty problem");
  STLLM_CHECK_ARG(D == kDecD, "stllm_attention_decode: head_dim %d != 128", D);
  STLLM_CHECK_ARG(dtype == STLLM_BF16 || dtype == STLLM_F16, "stllm_attention_decode: 16-bit dtypes only");
  STLLM_CHECK_ARG(((uintptr_t)q & 3) == 0 && ((uintptr_t)k & 3) == 0 && ((uintptr_t)v & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
                      q_bs % 2 == 0 && k_bs % 2 == 0 && k_rs % 2 == 0 && v_bs % 2 == 0 && v_rs % 2 == 0 && o_bs % 2 == 0,
                  "stllm_attention_decode: pointers / strides must be 4-byte aligned");
  const int nsplit = decode_splits(Skv);
  STLLM_CHECK_ARG(workspace_bytes >= stllm_attention_decode_workspace_bytes(B, H, Skv) && aligned16(workspace),
                  "stllm_attention_decode: workspace too small or misaligned");
  AttnParams p{};
  p.q = (const char*)q; p.q_bs = q_bs;
  p.k = (const char*)k; p.k_bs = k_bs; p.k_rs = k_rs;
  p.v = (const char*)v; p.v_bs = v_bs; p.v_rs = v_rs;
  p.o = (char*)out; p.o_bs = o_bs;
  p.B = B; p.H = H; p.Sq = 1; p.Skv = Skv; p.D = D;
  p.scale = scale; p.scale_log2 = scale * 1.44269504088896340736f;
  if ((Skv <= kDecSingleMax || B * H >= 256) && aligned16(q) && aligned16(k) && aligned16(v) && q_bs % 8 == 0 && k_bs % 8 == 0 &&
      k_rs % 8 == 0 && v_bs % 8 == 0 && v_rs % 8 == 0 && stllm_options().attn_decode_single) {
    if (dtype == STLLM_BF16) hipLaunchKernelGGL(attn_decode_single_kernel<bf16_t>, dim3(H, B), dim3(64 * kDecWaves), 0, stream, p);
    else hipLaunchKernelGGL(attn_decode_single_kernel<f16_t>, dim3(H, B), dim3(64 * kDecWaves), 0, stream, p);
    STLLM_CHECK_LAUNCH("stllm_attention_decode(single)");
    return STLLM_OK;
  }
  float* ws = reinterpret_cast<float*>(workspace);
  const int kps = (Skv + nsplit - 1) / nsplit;
  if (dtype == STLLM_BF16) {
    hipLaunchKernelGGL(attn_decode_partial_kernel<bf16_t>, dim3(nsplit, H, B), dim3(256), 0, stream, p, ws, nsplit, kps);
    hipLaunchKernelGGL(attn_decode_merge_kernel<bf16_t>, dim3(H, B), dim3(64), 0, stream, p, ws, nsplit);
  } else {
    hipLaunchKernelGGL(attn_decode_partial_kernel<f16_t>, dim3(nsplit, H, B), dim3(256), 0, stream, p, ws, nsplit, kps);
    hipLaunchKernelGGL(attn_decode_merge_kernel<f16_t>, dim3(H, B), dim3(64), 0, stream, p, ws, nsplit);
  }
  STLLM_CHECK_LAUNCH("stllm_attention_decode");
  return STLLM_OK;
}

extern "C" int64_t stllm_attention_decode_ragged_workspace_bytes(int B, int H, int max_kv) {
  return stllm_attention_decode_workspace_bytes(B, H, max_kv);
}

// stllm_attention_decode with per-row lengths: row b attends keys [0, min(kv_len[b], max_kv)).  The schedule (single pass | split-KV pair) and the grid come
// from max_kv exactly as stllm_attention_decode derives them from Skv; the per-row bounds live in the kernels.
extern "C" int stllm_attention_decode_ragged(int dtype, const void* q, int64_t q_bs, const void* k, int64_t k_bs, int64_t k_rs,
                                             const void* v, int64_t v_bs, int64_t v_rs, void* out, int64_t o_bs, int B, int H,
                                             const int32_t* kv_len, int max_kv, int D, float scale, void* workspace,
                                             int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(q && k && v && out && workspace && kv_len, "stllm_attention_decode_ragged: null pointer");
  STLLM_CHECK_ARG(B > 0 && H > 0 && max_kv > 0, "stllm_attention_decode_ragged: empty problem");
  if (D != kDecD || (dtype != STLLM_BF16 && dtype != STLLM_F16)) {
    stllm_set_error("stllm_attention_decode_ragged: head_dim %d / dtype %d unsupported (bf16 / fp16 at head_dim 128; fp32: stllm_attention with kv_len)", D, dtype);
    return STLLM_ERR_UNSUPPORTED;
  }
  STLLM_CHECK_ARG(((uintptr_t)q & 3) == 0 && ((uintptr_t)k & 3) == 0 && ((uintptr_t)v & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
                      ((uintptr_t)kv_len & 3) == 0 && q_bs % 2 == 0 && k_bs % 2 == 0 && k_rs % 2 == 0 && v_bs % 2 == 0 && v_rs % 2 == 0 && o_bs % 2 == 0,
                  "stllm_attention_decode_ragged: pointers / strides must be 4-byte aligned");
  const int nsplit = decode_splits(max_kv);
  STLLM_CHECK_ARG(workspace_bytes >= stllm_attention_decode_ragged_workspace_bytes(B, H, max_kv) && aligned16(workspace),
                  "stllm_attention_decode_ragged: workspace too small or misaligned");
  AttnParams p{};
  p.q = (const char*)q; p.q_bs = q_bs;
  p.k = (const char*)k; p.k_bs = k_bs; p.k_rs = k_rs;
  p.v = (const char*)v; p.v_bs = v_bs; p.v_rs = v_rs;
  p.o = (char*)out; p.o_bs = o_bs;
  p.B = B; p.H = H; p.Sq = 1; p.Skv = max_kv; p.D = D;
  p.scale = scale; p.scale_log2 = scale * 1.44269504088896340736f;
  p.kv_len = kv_len;
  if ((max_kv <= kDecSingleMax || B * H >= 256) && aligned16(q) && aligned16(k) && aligned16(v) && q_bs % 8 == 0 && k_bs % 8 == 0 &&
      k_rs % 8 == 0 && v_bs % 8 == 0 && v_rs % 8 == 0 && stllm_options().attn_decode_single) {
    if (dtype == STLLM_BF16) hipLaunchKernelGGL(attn_decode_single_ragged_kernel<bf16_t>, dim3(H, B), dim3(64 * kDecWaves), 0, stream, p);
    else hipLaunchKernelGGL(attn_decode_single_ragged_kernel<f16_t>, dim3(H, B), dim3(64 * kDecWaves), 0, stream, p);
    STLLM_CHECK_LAUNCH("stllm_attention_decode_ragged(single)");
    return STLLM_OK;
  }
  float* ws = reinterpret_cast<float*>(workspace);
  if (dtype == STLLM_BF16) {
    hipLaunchKernelGGL(attn_decode_partial_ragged_kernel<bf16_t>, dim3(nsplit, H, B), dim3(256), 0, stream, p, ws, nsplit);
    hipLaunchKernelGGL(attn_decode_merge_ragged_kernel<bf16_t>, dim3(H, B), dim3(64), 0, stream, p, ws, nsplit);
  } else {
    hipLaunchKernelGGL(attn_decode_partial_ragged_kernel<f16_t>, dim3(nsplit, H, B), dim3(256), 0, stream, p, ws, nsplit);
    hipLaunchKernelGGL(attn_decode_merge_ragged_kernel<f16_t>, dim3(H, B), dim3(64), 0, stream, p, ws, nsplit);
  }
  STLLM_CHECK_LAUNCH("stllm_attention_decode_ragged");
  return STLLM_OK;
}

// =====================================================================================================
// Shared-prefix attention: B = G * R query rows in G contiguous groups; the R rows of group g read the SAME P prefix keys (row g of
// the prefix buffers, never written) and each row b its own suffix keys [0, sfx_len[b]) (row b of the suffix buffers).
//   decode (Sq = 1, 16-bit): attn_shared_decode_kernel + attn_shared_merge_kernel, two launches.
//     prefix workgroups — one per (g, h, 32-row query tile, key range): 4 waves on disjoint 32-key tiles of the range (wave w: tiles w, w + 4, ...).  A wave
//       loads a K / V tile ONCE and applies it to all (<= 32) queries of the tile on the matrix cores: S^T = K . Q^T with the K rows as the A operand straight
//       from global memory (lane = key row: the fragment a lane needs is 16 contiguous bytes of its row), V^T through a wave-private LDS tile (the transposed
//       store of attn_mfma_kernel), the online softmax of attn_mfma_kernel per lane (= per query).  The next tile's loads are issued between the S^T chain
//       and the softmax.  Keys at or behind P are neither loaded nor counted.  The four wave states merge through LDS in a fixed order (2 <- 3 | 0 <- 1 ... see
//       below) and leave ONE record per (query row, range).
//     suffix workgroups — further blockIdx.x values of the same launch: the loop of decode_partial_body over keys [s * kps_s, ...) of row b's own suffix
//       (VALU; a copy, because the record layout differs and the ragged kernels' instruction streams are not to change).
//     records: kSplRec floats, O[128] | m | l, with m in the LOG2 domain (raw maximum * scale * log2 e) in this path.
//   extend (Sq > 1, 16-bit): attn_mfma_kernel<T, 128, NW, SPLIT> twice — the prefix as a non-causal problem of batch G with R * Sq query rows, the suffix
//     per row (causal, q_off = sfx_q_off, kv_len = sfx_len, LIVE loads) — and the same merge (their records keep RAW maxima: m_mult = scale * log2 e).
//   fp32 (verify mode, any Sq): attn_shared_f32_kernel, one workgroup per (b, i, h), a two-source key loop on the VALU.
// The merge folds a query row's prefix ranges, then its suffix records, in ascending order: deterministic, no atomics, no flags.
// =====================================================================================================
namespace {

struct SharedParams {
  const char* q; int64_t q_bs, q_rs;
  const char* kp; int64_t kp_bs, kp_rs;
  const char* vp; int64_t vp_bs, vp_rs;
  const char* ks; int64_t ks_bs, ks_rs;
  const char* vs; int64_t vs_bs, vs_rs;
  char* o; int64_t o_bs, o_rs;
  const int32_t* sfx_len;
  int max_sfx, sfx_q_off;
  int B, G, R, H, Sq, P;
  float scale_log2;
  int causal;
  float* ws_p; float* ws_s;             // prefix records [G][H][R * Sq][n_p], suffix records [B][H][Sq][n_s]
  int nsp, kps, qtiles, nss, kps_s;     // decode plan (shared_plan)
  float m_mult;                         // merge: log2-domain maximum = record maximum * m_mult
};

// key ranges of the decode pass: a pure function of (G, H, R, P) / of max_sfx, shared by the workspace query and the launch.  Prefix ranges are whole
// 32-key tiles, four tiles (one per wave) or more each, at most 32 ranges, enough of them for ~512 workgroups; suffix ranges hold ~64 keys, at most 8.
struct SharedPlan { int nsp, kps, qtiles, nss, kps_s; };
SharedPlan shared_plan(int G, int H, int R, int P, int max_sfx) {
  SharedPlan pl;
  pl.qtiles = (R + 31) / 32;
  const int tiles = (P + 31) / 32;
  const int64_t wgs = (int64_t)G * H * pl.qtiles;
  int want = (int)((512 + wgs - 1) / wgs);
  if (want > 32) want = 32;
  if (want > (tiles + 3) / 4) want = (tiles + 3) / 4;
  if (want < 1) want = 1;
  const int tps = (tiles + want - 1) / want;
  pl.kps = tps * 32;
  pl.nsp = (tiles + tps - 1) / tps;
  int ns = (max_sfx + 63) / 64;
  pl.nss = ns < 1 ? 1 : (ns > 8 ? 8 : ns);
  pl.kps_s = (max_sfx + pl.nss - 1) / pl.nss;
  if (pl.kps_s < 1) pl.kps_s = 1;
  return pl;
}

constexpr int kShVPitch = 32 * 2 + 8;                  // bytes per V^T row of a wave's LDS tile (attn_mfma_kernel's VPITCH)
constexpr int kShLds = 4 * kDecD * kShVPitch;          // 36864 bytes: four wave-private V^T tiles; reused by the wave merge (2 x 66 x 64 floats) and the suffix body

template <typename T>
__device__ __forceinline__ void shared_suffix_body(const SharedParams& p, float* __restrict__ lds_f, int b, int h, int sp) {
  float (*part)[kSplRec] = reinterpret_cast<float (*)[kSplRec]>(lds_f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int len = p.sfx_len ? min(p.sfx_len[b], p.max_sfx) : p.max_sfx;
  if (p.causal) len = min(len, p.sfx_q_off + 1);
  const int k0 = sp * p.kps_s, k1 = min(len, k0 + p.kps_s);
  float q0, q1;
  widen2<T>(*reinterpret_cast<const uint32_t*>(p.q + ((int64_t)b * p.q_bs + (int64_t)h * kDecD + 2 * lane) * 2), q0, q1);
  q0 *= p.scale_log2;
  q1 *= p.scale_log2;
  const char* kb = p.ks + ((int64_t)b * p.ks_bs + (int64_t)h * kDecD + 2 * lane) * 2;
  const char* vb = p.vs + ((int64_t)b * p.vs_bs + (int64_t)h * kDecD + 2 * lane) * 2;
  float m = kNeg, l = 0.0f, o0 = 0.0f, o1 = 0.0f;
  for (int key = k0 + wave; key < k1; key += 4) {
    float ka, kc, va, vc;
    widen2<T>(*reinterpret_cast<const uint32_t*>(kb + (int64_t)key * p.ks_rs * 2), ka, kc);
    widen2<T>(*reinterpret_cast<const uint32_t*>(vb + (int64_t)key * p.vs_rs * 2), va, vc);
    const float s = wave_sum(fmaf(q0, ka, q1 * kc));   // log2-domain score, identical in every lane
    const float mn = fmaxf(m, s);
    const float alpha = __builtin_amdgcn_exp2f(m - mn), pr = __builtin_amdgcn_exp2f(s - mn);
    l = fmaf(l, alpha, pr);
    o0 = fmaf(o0, alpha, pr * va);
    o1 = fmaf(o1, alpha, pr * vc);
    m = mn;
  }
  if (lane == 0) { part[wave][128] = m; part[wave][129] = l; }
  part[wave][2 * lane] = o0;
  part[wave][2 * lane + 1] = o1;
  __syncthreads();
  if (wave == 0) {
    const float mm = fmaxf(fmaxf(part[0][128], part[1][128]), fmaxf(part[2][128], part[3][128]));
    float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = __builtin_amdgcn_exp2f(part[w][128] - mm);   // a wave without keys: exp2(-huge) == 0 (all four empty: 1 * 0)
      ll = fmaf(part[w][129], f, ll);
      a0 = fmaf(part[w][2 * lane], f, a0);
      a1 = fmaf(part[w][2 * lane + 1], f, a1);
    }
    float* rec = p.ws_s + (((int64_t)b * p.H + h) * p.nss + sp) * kSplRec;
    rec[2 * lane] = a0;
    rec[2 * lane + 1] = a1;
    if (lane == 0) { rec[128] = mm; rec[129] = ll; }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void attn_shared_decode_kernel(const SharedParams p) {
  __shared__ __attribute__((aligned(16))) char lds[kShLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int n_prefix = p.G * p.H * p.qtiles * p.nsp;
  int id = blockIdx.x;
  if (id >= n_prefix) {   // workgroup-uniform
    id -= n_prefix;
    const int sp = id % p.nss;
    id /= p.nss;
    shared_suffix_body<T>(p, reinterpret_cast<float*>(lds), id / p.H, id % p.H, sp);
    return;
  }
  const int range = id % p.nsp;
  id /= p.nsp;
  const int qt = id % p.qtiles;
  id /= p.qtiles;
  const int h = id % p.H, g = id / p.H;
  const int k0 = range * p.kps, k1 = min(p.P, k0 + p.kps);   // k1 > k0 by the plan
  const int nt = (k1 - k0 + 31) >> 5;                        // 32-key tiles of the range; wave w walks tiles w, w + 4, ...
  const int iters = (nt + 3) >> 2;
  const int r = qt * 32 + li;                                // this lane's query: row r of the group
  const bool qlive = r < p.R;

  // ---- Q fragments (B operand of S^T): lane holds Q[r][ks*16 + lh*8 .. +8]; padding rows hold zeros and write nothing ----
  i32x4 qf[8];
  {
    const char* qp = p.q + ((int64_t)(g * p.R + (qlive ? r : 0)) * p.q_bs + (int64_t)h * kDecD + lh * 8) * 2;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const i32x4 z = {0, 0, 0, 0};
      qf[ks] = qlive ? *reinterpret_cast<const i32x4*>(qp + ks * 32) : z;
    }
  }
  f32x16 o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[i][e] = 0.0f;
  float m_run = kNeg, l_run = 0.0f;

  // lane (li, lh) owns key row kv0 + li of a tile: its 16-byte chunks c*16 + lh*8 (c = 0..7) are the K fragments of the S^T chain (A operand, k-step c)
  // and the V chunks 2c + lh of the transposed LDS store.  A row at or behind k1 (= P in the last tile of the last range) is NOT loaded.
  const char* kbase = p.kp + ((int64_t)g * p.kp_bs + (int64_t)h * kDecD + lh * 8) * 2;
  const char* vbase = p.vp + ((int64_t)g * p.vp_bs + (int64_t)h * kDecD + lh * 8) * 2;
  char* v_lds = lds + wave * (kDecD * kShVPitch);
  i32x4 kreg[8], vreg[8];
  auto load_tile = [&](int kv0) {
    const int kv = kv0 + li;
    const bool ok = kv < k1;
    const char* kr = kbase + (int64_t)kv * p.kp_rs * 2;
    const char* vr = vbase + (int64_t)kv * p.vp_rs * 2;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const i32x4 z = {0, 0, 0, 0};
      kreg[c] = ok ? *reinterpret_cast<const i32x4*>(kr + c * 32) : z;
      vreg[c] = ok ? *reinterpret_cast<const i32x4*>(vr + c * 32) : z;
    }
  };
  int t = wave;
  if (t < nt) load_tile(k0 + t * 32);
  for (int it = 0; it < iters; ++it, t += 4) {
    const bool act = t < nt;            // wave-uniform; every wave keeps the barriers of all `iters` rounds
    const int kv0 = k0 + t * 32;
    __syncthreads();                    // the wave's previous V^T tile is consumed
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.0f;
    if (act) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int cc = 2 * c + lh;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t w = (uint32_t)vreg[c][e];
          *reinterpret_cast<uint16_t*>(v_lds + (cc * 8 + 2 * e) * kShVPitch + li * 2) = (uint16_t)(w & 0xffff);
          *reinterpret_cast<uint16_t*>(v_lds + (cc * 8 + 2 * e + 1) * kShVPitch + li * 2) = (uint16_t)(w >> 16);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) s = Elem<T>::mfma(kreg[ks], qf[ks], s);   // S^T[key][query]
    }
    if (t + 4 < nt) load_tile(k0 + (t + 4) * 32);   // in flight under the softmax and the P V chain
    __syncthreads();
    if (!act) continue;
    if (kv0 + 32 > k1) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int kv = kv0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        s[e] = kv >= k1 ? kNeg : s[e];
      }
    }
    float mx = s[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s[e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float mc = m_new * p.scale_log2;
    float rs = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pv = __builtin_amdgcn_exp2f(fmaf(s[e], p.scale_log2, -mc));   // masked: exp2(-huge) == 0
      s[e] = pv;
      rs += pv;
    }
    rs += __shfl_xor(rs, 32, 64);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);
    l_run = fmaf(l_run, alpha, rs);
    m_run = m_new;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[i][e] *= alpha;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      i32x4 pf;
#pragma unroll
      for (int e = 0; e < 4; ++e) pf[e] = (int)(Elem<T>::pack2(s[a * 8 + 2 * e], s[a * 8 + 2 * e + 1]));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const char* vp = v_lds + (i * 32 + li) * kShVPitch + (16 * a + 4 * lh) * 2;
        const i32x2 lo = *reinterpret_cast<const i32x2*>(vp);
        const i32x2 hi = *reinterpret_cast<const i32x2*>(vp + 16);
        const i32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
        o[i] = Elem<T>::mfma(vf, pf, o[i]);
      }
    }
  }

  // ---- the four wave states -> one: 0 <- 2 and 1 <- 3, then 0 <- 1, through two slots of [66][64] floats (lane-major: every lane reads back what the same
  // lane of the other wave wrote).  A fixed order; a wave that walked no tile holds the empty state (m = kNeg, l = 0, O = 0) and weighs exp2(-huge) = 0 ----
  float* st = reinterpret_cast<float*>(lds);
  auto put = [&](int slot) {
    float* d = st + slot * (66 * 64) + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) d[(i * 16 + e) * 64] = o[i][e];
    d[64 * 64] = m_run;
    d[65 * 64] = l_run;
  };
  auto take = [&](int slot) {
    const float* d = st + slot * (66 * 64) + lane;
    const float mb = d[64 * 64], lb = d[65 * 64];
    const float mn = fmaxf(m_run, mb);
    const float fa = __builtin_amdgcn_exp2f((m_run - mn) * p.scale_log2), fb = __builtin_amdgcn_exp2f((mb - mn) * p.scale_log2);
    l_run = fmaf(l_run, fa, lb * fb);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[i][e] = fmaf(o[i][e], fa, d[(i * 16 + e) * 64] * fb);
    m_run = mn;
  };
  __syncthreads();
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) take(wave);
  __syncthreads();
  if (wave == 1) put(0);
  __syncthreads();
  if (wave != 0) return;
  take(0);
  if (!qlive) return;   // padding query rows write no record
  float* rec = p.ws_p + ((((int64_t)g * p.H + h) * p.R + r) * p.nsp + range) * kSplRec;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const f32x4 ov = {o[i][4 * gq + 0], o[i][4 * gq + 1], o[i][4 * gq + 2], o[i][4 * gq + 3]};
      *reinterpret_cast<f32x4*>(rec + i * 32 + 8 * gq + 4 * lh) = ov;
    }
  if (lh == 0) { rec[128] = m_run * p.scale_log2; rec[129] = l_run; }
}

// one workgroup (one wave) per query row (b, i, h): n_p prefix records of its group row, then n_s suffix records of its own row, ascending
template <typename T>
__global__ __launch_bounds__(64) void attn_shared_merge_kernel(const SharedParams p, int n_p, int n_s) {
  const int lane = threadIdx.x, i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int g = b / p.R, rr = b - g * p.R;
  const float* ra = p.ws_p + ((((int64_t)g * p.H + h) * ((int64_t)p.R * p.Sq) + (int64_t)rr * p.Sq + i) * n_p) * kSplRec;
  const float* rb = p.ws_s + ((((int64_t)b * p.H + h) * p.Sq + i) * n_s) * kSplRec;
  float mm = kNeg * 2.0f;
  for (int s = 0; s < n_p; ++s) mm = fmaxf(mm, ra[s * kSplRec + 128] * p.m_mult);
  for (int s = 0; s < n_s; ++s) mm = fmaxf(mm, rb[s * kSplRec + 128] * p.m_mult);
  float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
  for (int s = 0; s < n_p; ++s) {
    const float f = __builtin_amdgcn_exp2f(ra[s * kSplRec + 128] * p.m_mult - mm);   // empty records: exp2(-huge) == 0
    ll = fmaf(ra[s * kSplRec + 129], f, ll);
    a0 = fmaf(ra[s * kSplRec + 2 * lane], f, a0);
    a1 = fmaf(ra[s * kSplRec + 2 * lane + 1], f, a1);
  }
  for (int s = 0; s < n_s; ++s) {
    const float f = __builtin_amdgcn_exp2f(rb[s * kSplRec + 128] * p.m_mult - mm);
    ll = fmaf(rb[s * kSplRec + 129], f, ll);
    a0 = fmaf(rb[s * kSplRec + 2 * lane], f, a0);
    a1 = fmaf(rb[s * kSplRec + 2 * lane + 1], f, a1);
  }
  const float inv = 1.0f / ll;
  uint32_t* op = reinterpret_cast<uint32_t*>(p.o + ((int64_t)b * p.o_bs + (int64_t)i * p.o_rs + (int64_t)h * kDecD + 2 * lane) * 2);
  *op = Elem<T>::pack2(a0 * inv, a1 * inv);
}

// fp32 (the verify mode): one workgroup per (b, i, h); wave w takes keys w, w + 4, ... of the row's P + n_s keys (prefix first), lane l the dims 2l, 2l + 1
__global__ __launch_bounds__(256) void attn_shared_f32_kernel(const SharedParams p) {
  __shared__ float part[4][kSplRec];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int g = b / p.R;
  int ns = p.sfx_len ? min(p.sfx_len[b], p.max_sfx) : p.max_sfx;
  if (p.causal) ns = min(ns, p.sfx_q_off + i + 1);
  if (ns < 0) ns = 0;
  const f32x2 qv = *reinterpret_cast<const f32x2*>(reinterpret_cast<const float*>(p.q) + (int64_t)b * p.q_bs + (int64_t)i * p.q_rs + (int64_t)h * kDecD + 2 * lane);
  const float q0 = qv[0] * p.scale_log2, q1 = qv[1] * p.scale_log2;
  const float* kpf = reinterpret_cast<const float*>(p.kp) + (int64_t)g * p.kp_bs + (int64_t)h * kDecD + 2 * lane;
  const float* vpf = reinterpret_cast<const float*>(p.vp) + (int64_t)g * p.vp_bs + (int64_t)h * kDecD + 2 * lane;
  const float* ksf = reinterpret_cast<const float*>(p.ks) + (int64_t)b * p.ks_bs + (int64_t)h * kDecD + 2 * lane;
  const float* vsf = reinterpret_cast<const float*>(p.vs) + (int64_t)b * p.vs_bs + (int64_t)h * kDecD + 2 * lane;
  float m = kNeg, l = 0.0f, o0 = 0.0f, o1 = 0.0f;
  const int total = p.P + ns;
  for (int j = wave; j < total; j += 4) {
    const bool pre = j < p.P;
    const f32x2 kk = *reinterpret_cast<const f32x2*>(pre ? kpf + (int64_t)j * p.kp_rs : ksf + (int64_t)(j - p.P) * p.ks_rs);
    const f32x2 vv = *reinterpret_cast<const f32x2*>(pre ? vpf + (int64_t)j * p.vp_rs : vsf + (int64_t)(j - p.P) * p.vs_rs);
    const float s = wave_sum(fmaf(q0, kk[0], q1 * kk[1]));
    const float mn = fmaxf(m, s);
    const float alpha = __builtin_amdgcn_exp2f(m - mn), pr = __builtin_amdgcn_exp2f(s - mn);
    l = fmaf(l, alpha, pr);
    o0 = fmaf(o0, alpha, pr * vv[0]);
    o1 = fmaf(o1, alpha, pr * vv[1]);
    m = mn;
  }
  if (lane == 0) { part[wave][128] = m; part[wave][129] = l; }
  part[wave][2 * lane] = o0;
  part[wave][2 * lane + 1] = o1;
  __syncthreads();
  if (wave == 0) {
    const float mm = fmaxf(fmaxf(part[0][128], part[1][128]), fmaxf(part[2][128], part[3][128]));
    float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = __builtin_amdgcn_exp2f(part[w][128] - mm);
      ll = fmaf(part[w][129], f, ll);
      a0 = fmaf(part[w][2 * lane], f, a0);
      a1 = fmaf(part[w][2 * lane + 1], f, a1);
    }
    const f32x2 r = {a0 / ll, a1 / ll};
    *reinterpret_cast<f32x2*>(reinterpret_cast<float*>(p.o) + (int64_t)b * p.o_bs + (int64_t)i * p.o_rs + (int64_t)h * kDecD + 2 * lane) = r;
  }
}

template <typename T, int NW, bool LIVE>
void launch_shared_pass_nw(const AttnParams& a, const KsplitPlan& pl, hipStream_t stream) {
  hipLaunchKernelGGL((attn_mfma_kernel<T, 128, NW, true, LIVE>), dim3(pl.chunks * pl.nsplit, a.H, a.B), dim3(64 * NW), 0, stream, a);
}
template <typename T, bool LIVE>
void launch_shared_pass(AttnParams a, const KsplitPlan& pl, hipStream_t stream) {
  a.nsplit = pl.nsplit;
  a.kps = pl.kps;
  switch (pl.nw) {
    case 1: launch_shared_pass_nw<T, 1, LIVE>(a, pl, stream); break;
    case 2: launch_shared_pass_nw<T, 2, LIVE>(a, pl, stream); break;
    case 3: launch_shared_pass_nw<T, 3, LIVE>(a, pl, stream); break;
    default: launch_shared_pass_nw<T, 4, LIVE>(a, pl, stream); break;
  }
}

template <typename T>
int launch_shared(SharedParams p, float scale, float* ws, hipStream_t stream) {
  if (p.Sq == 1) {
    const SharedPlan pl = shared_plan(p.G, p.H, p.R, p.P, p.max_sfx);
    p.nsp = pl.nsp; p.kps = pl.kps; p.qtiles = pl.qtiles; p.nss = pl.nss; p.kps_s = pl.kps_s;
    p.ws_p = ws;
    p.ws_s = ws + (int64_t)p.B * p.H * pl.nsp * kSplRec;
    p.m_mult = 1.0f;
    const int64_t wgs = (int64_t)p.G * p.H * pl.qtiles * pl.nsp + (int64_t)p.B * p.H * pl.nss;
    hipLaunchKernelGGL(attn_shared_decode_kernel<T>, dim3((unsigned)wgs), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(attn_shared_merge_kernel<T>, dim3(1, p.H, p.B), dim3(64), 0, stream, p, pl.nsp, pl.nss);
    STLLM_CHECK_LAUNCH("stllm_attention_shared(decode)");
    stllm_set_last_kernel("attn_shared_decode_kernel");
    return STLLM_OK;
  }
  const KsplitPlan pa = ksplit_plan(p.G, p.H, p.R * p.Sq, p.P), pb = ksplit_plan(p.B, p.H, p.Sq, p.max_sfx);
  p.ws_p = ws;
  p.ws_s = ws + (int64_t)p.B * p.H * p.Sq * pa.nsplit * kSplRec;
  p.m_mult = p.scale_log2;
  AttnParams a{};
  a.q = p.q; a.q_bs = (int64_t)p.R * p.q_bs; a.q_rs = p.q_rs;       // the R * Sq query rows of a group at ONE row stride (checked by the caller)
  a.k = p.kp; a.k_bs = p.kp_bs; a.k_rs = p.kp_rs;
  a.v = p.vp; a.v_bs = p.vp_bs; a.v_rs = p.vp_rs;
  a.B = p.G; a.H = p.H; a.Sq = p.R * p.Sq; a.Skv = p.P; a.D = kDecD;
  a.scale = scale; a.scale_log2 = p.scale_log2;
  a.ws = p.ws_p;
  launch_shared_pass<T, false>(a, pa, stream);
  AttnParams s{};
  s.q = p.q; s.q_bs = p.q_bs; s.q_rs = p.q_rs;
  s.k = p.ks; s.k_bs = p.ks_bs; s.k_rs = p.ks_rs;
  s.v = p.vs; s.v_bs = p.vs_bs; s.v_rs = p.vs_rs;
  s.B = p.B; s.H = p.H; s.Sq = p.Sq; s.Skv = p.max_sfx; s.D = kDecD;
  s.scale = scale; s.scale_log2 = p.scale_log2;
  s.causal = p.causal; s.q_off = p.causal ? p.sfx_q_off : 0;
  s.kv_len = p.sfx_len;
  s.ws = p.ws_s;
  launch_shared_pass<T, true>(s, pb, stream);
  hipLaunchKernelGGL(attn_shared_merge_kernel<T>, dim3(p.Sq, p.H, p.B), dim3(64), 0, stream, p, pa.nsplit, pb.nsplit);
  STLLM_CHECK_LAUNCH("stllm_attention_shared(extend)");
  stllm_set_last_kernel("attn_shared_extend");
  return STLLM_OK;
}

// =====================================================================================================
// Packed segments on a shared base: the R segments of stllm_attention_segments, every one of them behind the SAME P prefix keys — ONE row of a
// base buffer that is never written — and its own suffix keys in row slot[r] of the slot buffers.  The tables are suffix-local (q_off_tab = sfx_off, kv_len = sfx_len).
//   16-bit: the extend scheme of launch_shared on a packed buffer, three launches — the prefix as ONE non-causal problem of T query rows and P keys
//     (attn_mfma_kernel<T, 128, NW, SPLIT>, full query tiles whatever the segments' lengths), the suffixes per segment (the SEG + SPLIT + LIVE instantiation of
//     stllm_attention_segments' key split, which always leaves records here) and attn_segments_shared_merge_kernel.
//   fp32: attn_segments_shared_f32_kernel, attn_shared_f32_kernel's two-source key loop addressed through the segment tables.
// Both new kernels take seg_row's guard first: a pad row or a bad segment returns before it reads a record or a key and writes nothing.
// =====================================================================================================
struct SegSharedParams {
  AttnSegParams seg;                    // q / o (packed), ks / vs as k / v, the four tables, T, n_slots, B = R, Sq = max_n, Skv = max_sfx, ws = suffix records, nsplit = their count
  const char* kp; int64_t kp_rs;        // the ONE prefix row
  const char* vp; int64_t vp_rs;
  int P;
  const float* ws_p; int n_p;           // prefix records [H][T][n_p]
  float m_mult;                         // merge: log2-domain maximum = record maximum * m_mult (the records keep RAW maxima)
};

// one workgroup (one wave) per (query row i, head, segment r): attn_shared_merge_kernel's fold — the n_p prefix records of packed row row0[r] + i, then the
// n_s suffix records of (r, i), ascending — in the same arithmetic and the same order
template <typename T>
__global__ __launch_bounds__(64) void attn_segments_shared_merge_kernel(const SegSharedParams p) {
  const int lane = threadIdx.x, i = blockIdx.x, h = blockIdx.y, r = blockIdx.z;
  const SegRow s = seg_row(p.seg, r);
  if (i >= s.n) return;
  const int n_p = p.n_p, n_s = p.seg.nsplit;
  const int64_t row = (int64_t)s.row0 + i;
  const float* ra = p.ws_p + (((int64_t)h * p.seg.T + row) * n_p) * kSplRec;
  const float* rb = p.seg.ws + ((((int64_t)r * p.seg.H + h) * p.seg.Sq + i) * n_s) * kSplRec;
  float mm = kNeg * 2.0f;
  for (int c = 0; c < n_p; ++c) mm = fmaxf(mm, ra[c * kSplRec + 128] * p.m_mult);
  for (int c = 0; c < n_s; ++c) mm = fmaxf(mm, rb[c * kSplRec + 128] * p.m_mult);
  float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
  for (int c = 0; c < n_p; ++c) {
    const float f = __builtin_amdgcn_exp2f(ra[c * kSplRec + 128] * p.m_mult - mm);   // empty records: exp2(-huge) == 0
    ll = fmaf(ra[c * kSplRec + 129], f, ll);
    a0 = fmaf(ra[c * kSplRec + 2 * lane], f, a0);
    a1 = fmaf(ra[c * kSplRec + 2 * lane + 1], f, a1);
  }
  for (int c = 0; c < n_s; ++c) {
    const float f = __builtin_amdgcn_exp2f(rb[c * kSplRec + 128] * p.m_mult - mm);
    ll = fmaf(rb[c * kSplRec + 129], f, ll);
    a0 = fmaf(rb[c * kSplRec + 2 * lane], f, a0);
    a1 = fmaf(rb[c * kSplRec + 2 * lane + 1], f, a1);
  }
  const float inv = 1.0f / ll;
  uint32_t* op = reinterpret_cast<uint32_t*>(p.seg.o + (row * p.seg.o_rs + (int64_t)h * kDecD + 2 * lane) * 2);
  *op = Elem<T>::pack2(a0 * inv, a1 * inv);
}

// fp32 (the verify mode): one workgroup per (i, h, r); wave w takes keys w, w + 4, ... of the P prefix keys and the suffix keys j <= sfx_off + i (prefix first)
__global__ __launch_bounds__(256) void attn_segments_shared_f32_kernel(const SegSharedParams p) {
  __shared__ float part[4][kSplRec];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x, h = blockIdx.y, r = blockIdx.z;
  const SegRow s = seg_row(p.seg, r);
  if (i >= s.n) return;   // workgroup-uniform: nobody waits at the barrier below
  const int ns = min(s.kvlen, s.q_off + i + 1);
  const int64_t row = (int64_t)s.row0 + i;
  const f32x2 qv = *reinterpret_cast<const f32x2*>(reinterpret_cast<const float*>(p.seg.q) + row * p.seg.q_rs + (int64_t)h * kDecD + 2 * lane);
  const float q0 = qv[0] * p.seg.scale_log2, q1 = qv[1] * p.seg.scale_log2;
  const float* kpf = reinterpret_cast<const float*>(p.kp) + (int64_t)h * kDecD + 2 * lane;
  const float* vpf = reinterpret_cast<const float*>(p.vp) + (int64_t)h * kDecD + 2 * lane;
  const float* ksf = reinterpret_cast<const float*>(p.seg.k) + (int64_t)s.slot * p.seg.k_bs + (int64_t)h * kDecD + 2 * lane;
  const float* vsf = reinterpret_cast<const float*>(p.seg.v) + (int64_t)s.slot * p.seg.v_bs + (int64_t)h * kDecD + 2 * lane;
  float m = kNeg, l = 0.0f, o0 = 0.0f, o1 = 0.0f;
  const int total = p.P + ns;
  for (int j = wave; j < total; j += 4) {
    const bool pre = j < p.P;
    const f32x2 kk = *reinterpret_cast<const f32x2*>(pre ? kpf + (int64_t)j * p.kp_rs : ksf + (int64_t)(j - p.P) * p.seg.k_rs);
    const f32x2 vv = *reinterpret_cast<const f32x2*>(pre ? vpf + (int64_t)j * p.vp_rs : vsf + (int64_t)(j - p.P) * p.seg.v_rs);
    const float sc = wave_sum(fmaf(q0, kk[0], q1 * kk[1]));
    const float mn = fmaxf(m, sc);
    const float alpha = __builtin_amdgcn_exp2f(m - mn), pr = __builtin_amdgcn_exp2f(sc - mn);
    l = fmaf(l, alpha, pr);
    o0 = fmaf(o0, alpha, pr * vv[0]);
    o1 = fmaf(o1, alpha, pr * vv[1]);
    m = mn;
  }
  if (lane == 0) { part[wave][128] = m; part[wave][129] = l; }
  part[wave][2 * lane] = o0;
  part[wave][2 * lane + 1] = o1;
  __syncthreads();
  if (wave == 0) {
    const float mm = fmaxf(fmaxf(part[0][128], part[1][128]), fmaxf(part[2][128], part[3][128]));
    float ll = 0.0f, a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = __builtin_amdgcn_exp2f(part[w][128] - mm);
      ll = fmaf(part[w][129], f, ll);
      a0 = fmaf(part[w][2 * lane], f, a0);
      a1 = fmaf(part[w][2 * lane + 1], f, a1);
    }
    const f32x2 res = {a0 / ll, a1 / ll};
    *reinterpret_cast<f32x2*>(reinterpret_cast<float*>(p.seg.o) + row * p.seg.o_rs + (int64_t)h * kDecD + 2 * lane) = res;
  }
}

// the suffix pass: launch_ksplit's partial launch on the SEG instantiation, without its merge
template <typename T>
void launch_segments_shared_suffix(AttnSegParams s, const KsplitPlan& pl, hipStream_t stream) {
  s.nsplit = pl.nsplit;
  s.kps = pl.kps;
  switch (pl.nw) {
    case 1: launch_ksplit_nw<T, 1, true, true>(s, pl, stream); break;
    case 2: launch_ksplit_nw<T, 2, true, true>(s, pl, stream); break;
    case 3: launch_ksplit_nw<T, 3, true, true>(s, pl, stream); break;
    default: launch_ksplit_nw<T, 4, true, true>(s, pl, stream); break;
  }
}

template <typename T>
int launch_segments_shared(SegSharedParams p, float* ws, hipStream_t stream) {
  const AttnSegParams& g = p.seg;
  const KsplitPlan pa = ksplit_plan(1, g.H, g.T, p.P), pb = ksplit_plan(g.B, g.H, g.Sq, g.Skv);
  float* ws_p = ws;
  float* ws_s = ws + (int64_t)g.H * g.T * pa.nsplit * kSplRec;
  AttnParams a{};
  a.q = g.q; a.q_bs = 0; a.q_rs = g.q_rs;                  // the T packed rows are ONE batch row of query rows
  a.k = p.kp; a.k_bs = 0; a.k_rs = p.kp_rs;
  a.v = p.vp; a.v_bs = 0; a.v_rs = p.vp_rs;
  a.B = 1; a.H = g.H; a.Sq = g.T; a.Skv = p.P; a.D = kDecD;   // Skv = P: key rows at or behind P are not loaded
  a.scale = g.scale; a.scale_log2 = g.scale_log2;
  a.ws = ws_p;
  launch_shared_pass<T, false>(a, pa, stream);
  STLLM_CHECK_LAUNCH("stllm_attention_segments_shared(prefix pass)");
  p.seg.ws = ws_s;
  launch_segments_shared_suffix<T>(p.seg, pb, stream);
  STLLM_CHECK_LAUNCH("stllm_attention_segments_shared(suffix pass)");
  p.seg.nsplit = pb.nsplit;
  p.ws_p = ws_p; p.n_p = pa.nsplit;
  p.m_mult = g.scale_log2;
  hipLaunchKernelGGL(attn_segments_shared_merge_kernel<T>, dim3(g.Sq, g.H, g.B), dim3(64), 0, stream, p);
  STLLM_CHECK_LAUNCH("stllm_attention_segments_shared(merge)");
  stllm_set_last_kernel("attn_segments_shared");
  return STLLM_OK;
}

}  // namespace

extern "C" int64_t stllm_attention_segments_shared_workspace_bytes(int R, int H, int T, int P, int max_n, int max_sfx) {
  if (R <= 0 || H <= 0 || T <= 0 || P <= 0 || max_n <= 0 || max_sfx <= 0) return -1;
  return ((int64_t)H * T * ksplit_plan(1, H, T, P).nsplit + (int64_t)R * H * max_n * ksplit_plan(R, H, max_n, max_sfx).nsplit) * kSplRec * 4;
}

extern "C" int stllm_attention_segments_shared(int dtype, const void* q, int64_t q_rs, const void* kp, int64_t kp_rs, const void* vp, int64_t vp_rs, int P,
                                               const void* ks, int64_t ks_bs, int64_t ks_rs, const void* vs, int64_t vs_bs, int64_t vs_rs, void* out,
                                               int64_t o_rs, int R, int H, int D, int T, int n_slots, int max_n, int max_sfx, float scale,
                                               const int32_t* slot, const int32_t* row0, const int32_t* sfx_off, const int32_t* sfx_len, void* workspace,
                                               int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(q && kp && vp && ks && vs && out && slot && row0 && sfx_off && sfx_len, "stllm_attention_segments_shared: null pointer");
  STLLM_CHECK_ARG(R > 0 && R <= 65535 && H > 0 && T > 0 && P > 0 && n_slots > 0 && max_n > 0 && max_sfx > 0,
                  "stllm_attention_segments_shared: empty problem (or R > 65535) (R %d, H %d, T %d, P %d, n_slots %d, max_n %d, max_sfx %d)",
                  R, H, T, P, n_slots, max_n, max_sfx);
  if (D != kDecD || (dtype != STLLM_BF16 && dtype != STLLM_F16 && dtype != STLLM_F32)) {
    stllm_set_error("stllm_attention_segments_shared: head_dim %d / dtype %d unsupported (bf16 / fp16 / fp32 at head_dim 128)", D, dtype);
    return STLLM_ERR_UNSUPPORTED;
  }
  STLLM_CHECK_ARG(aligned16(q) && aligned16(kp) && aligned16(vp) && aligned16(ks) && aligned16(vs) && aligned16(out),
                  "stllm_attention_segments_shared: pointers must be 16-byte aligned");
  STLLM_CHECK_ARG(q_rs % 8 == 0 && kp_rs % 8 == 0 && vp_rs % 8 == 0 && ks_bs % 8 == 0 && ks_rs % 8 == 0 && vs_bs % 8 == 0 && vs_rs % 8 == 0 && o_rs % 8 == 0,
                  "stllm_attention_segments_shared: strides must be multiples of 8 elements");
  STLLM_CHECK_ARG(((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(row0) | reinterpret_cast<uintptr_t>(sfx_off) |
                    reinterpret_cast<uintptr_t>(sfx_len)) & 3) == 0, "stllm_attention_segments_shared: tables must be 4-byte aligned");
  SegSharedParams p{};
  AttnSegParams& g = p.seg;
  g.q = (const char*)q; g.q_bs = 0; g.q_rs = q_rs;
  g.k = (const char*)ks; g.k_bs = ks_bs; g.k_rs = ks_rs;
  g.v = (const char*)vs; g.v_bs = vs_bs; g.v_rs = vs_rs;
  g.o = (char*)out; g.o_bs = 0; g.o_rs = o_rs;
  g.B = R; g.H = H; g.Sq = max_n; g.Skv = max_sfx; g.D = D;
  g.scale = scale; g.scale_log2 = scale * 1.44269504088896340736f;
  g.causal = 1; g.kv_len = sfx_len; g.q_off_tab = sfx_off;
  g.slot = slot; g.row0 = row0; g.T = T; g.n_slots = n_slots;
  p.kp = (const char*)kp; p.kp_rs = kp_rs;
  p.vp = (const char*)vp; p.vp_rs = vp_rs;
  p.P = P;
  if (dtype == STLLM_F32) {
    hipLaunchKernelGGL(attn_segments_shared_f32_kernel, dim3(max_n, H, R), dim3(256), 0, stream, p);
    STLLM_CHECK_LAUNCH("stllm_attention_segments_shared(fp32)");
    stllm_set_last_kernel("attn_segments_shared");
    return STLLM_OK;
  }
  STLLM_CHECK_ARG(workspace && aligned16(workspace) && workspace_bytes >= stllm_attention_segments_shared_workspace_bytes(R, H, T, P, max_n, max_sfx),
                  "stllm_attention_segments_shared: workspace too small or misaligned");
  float* ws = reinterpret_cast<float*>(workspace);
  return dtype == STLLM_BF16 ? launch_segments_shared<bf16_t>(p, ws, stream) : launch_segments_shared<f16_t>(p, ws, stream);
}

extern "C" int64_t stllm_attention_shared_workspace_bytes(int B, int G, int H, int Sq, int P, int max_sfx) {
  if (B <= 0 || G <= 0 || B % G != 0 || H <= 0 || Sq <= 0 || P <= 0 || max_sfx <= 0) return -1;
  const int R = B / G;
  if (Sq == 1) {
    const SharedPlan pl = shared_plan(G, H, R, P, max_sfx);
    return (int64_t)B * H * (pl.nsp + pl.nss) * kSplRec * 4;
  }
  return (int64_t)B * H * Sq * (ksplit_plan(G, H, R * Sq, P).nsplit + ksplit_plan(B, H, Sq, max_sfx).nsplit) * kSplRec * 4;
}

extern "C" int stllm_attention_shared(int dtype, const void* q, int64_t q_bs, int64_t q_rs, const void* kp, int64_t kp_bs, int64_t kp_rs,
                                      const void* vp, int64_t vp_bs, int64_t vp_rs, int P, const void* ks, int64_t ks_bs, int64_t ks_rs,
                                      const void* vs, int64_t vs_bs, int64_t vs_rs, const int32_t* sfx_len, int max_sfx, int sfx_q_off,
                                      void* out, int64_t o_bs, int64_t o_rs, int B, int G, int H, int Sq, int D, float scale, int causal,
                                      void* workspace, int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(q && kp && vp && ks && vs && out, "stllm_attention_shared: null pointer");
  STLLM_CHECK_ARG(B > 0 && G > 0 && B % G == 0 && H > 0 && Sq > 0 && P > 0 && max_sfx > 0 && sfx_q_off >= 0,
                  "stllm_attention_shared: needs B %% G == 0 and a non-empty prefix and suffix (B %d, G %d, H %d, Sq %d, P %d, max_sfx %d, sfx_q_off %d)", B, G, H, Sq, P, max_sfx, sfx_q_off);
  if (D != kDecD || (dtype != STLLM_BF16 && dtype != STLLM_F16 && dtype != STLLM_F32)) {
    stllm_set_error("stllm_attention_shared: head_dim %d / dtype %d unsupported (bf16 / fp16 / fp32 at head_dim 128)", D, dtype);
    return STLLM_ERR_UNSUPPORTED;
  }
  STLLM_CHECK_ARG(aligned16(q) && aligned16(kp) && aligned16(vp) && aligned16(ks) && aligned16(vs) && aligned16(out) && ((uintptr_t)sfx_len & 3) == 0,
                  "stllm_attention_shared: pointers must be 16-byte aligned");
  STLLM_CHECK_ARG(q_bs % 8 == 0 && q_rs % 8 == 0 && kp_bs % 8 == 0 && kp_rs % 8 == 0 && vp_bs % 8 == 0 && vp_rs % 8 == 0 && ks_bs % 8 == 0 && ks_rs % 8 == 0 &&
                      vs_bs % 8 == 0 && vs_rs % 8 == 0 && o_bs % 8 == 0 && o_rs % 8 == 0, "stllm_attention_shared: strides must be multiples of 8 elements");
  SharedParams p{};
  p.q = (const char*)q; p.q_bs = q_bs; p.q_rs = q_rs;
  p.kp = (const char*)kp; p.kp_bs = kp_bs; p.kp_rs = kp_rs;
  p.vp = (const char*)vp; p.vp_bs = vp_bs; p.vp_rs = vp_rs;
  p.ks = (const char*)ks; p.ks_bs = ks_bs; p.ks_rs = ks_rs;
  p.vs = (const char*)vs; p.vs_bs = vs_bs; p.vs_rs = vs_rs;
  p.o = (char*)out; p.o_bs = o_bs; p.o_rs = o_rs;
  p.sfx_len = sfx_len; p.max_sfx = max_sfx; p.sfx_q_off = sfx_q_off;
  p.B = B; p.G = G; p.R = B / G; p.H = H; p.Sq = Sq; p.P = P;
  p.scale_log2 = scale * 1.44269504088896340736f;
  p.causal = causal;
  if (dtype == STLLM_F32) {
    hipLaunchKernelGGL(attn_shared_f32_kernel, dim3(Sq, H, B), dim3(256), 0, stream, p);
    STLLM_CHECK_LAUNCH("stllm_attention_shared(fp32)");
    stllm_set_last_kernel("attn_shared_f32_kernel");
    return STLLM_OK;
  }
  if (Sq > 1 && p.R > 1 && q_bs != (int64_t)Sq * q_rs) {
    stllm_set_error("stllm_attention_shared: Sq > 1 in bf16 / fp16 needs the query rows of a group at one row stride (q_bs == Sq * q_rs; got %lld, %d x %lld)",
                    (long long)q_bs, Sq, (long long)q_rs);
    return STLLM_ERR_UNSUPPORTED;
  }
  STLLM_CHECK_ARG(workspace && aligned16(workspace) && workspace_bytes >= stllm_attention_shared_workspace_bytes(B, G, H, Sq, P, max_sfx),
                  "stllm_attention_shared: workspace too small or misaligned");
  float* ws = reinterpret_cast<float*>(workspace);
  return dtype == STLLM_BF16 ? launch_shared<bf16_t>(p, scale, ws, stream) : launch_shared<f16_t>(p, scale, ws, stream);
}

#ifdef STLLM_ATTN_TRACE
// trace build only: the stamps of the last launch(es) -> host (tools/attn_trace.py)
extern "C" int stllm_attn_trace_read(void* dst, int64_t bytes, int clear) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_attn_trace), (size_t)bytes) != hipSuccess) return -2;
  if (clear) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_attn_trace)) != hipSuccess || hipMemset(p, 0, sizeof(g_attn_trace)) != hipSuccess) return -3;
  }
  return 0;
}
#endif
