// Skinny GEMM for the decode regime:  C[M,N] = epilogue(A[M,K] @ W[N,K]^T) with M <= 4 (M <= 8 with
// stllm_set_option("gemm_gemv", 2): the 5 beams of demo.py's beam search; staged, off by default until timed), bf16 / fp16.
//
// One token per sequence means every weight matrix is streamed from HBM once per step and used for M <= 4 rows: the
// problem is HBM-bound (Vicuna-7B: 13.2 GB per token), the matrix cores are useless (a 64-row MFMA tile would be 98 % padding).
//   * A (M x K, <= 88 KB) is staged once per workgroup in LDS;
//   * every WAVE owns the column pair (c, c + 32) of a 64-column group — exactly the [32 gate | 32 up] / [x_lo | x_hi]
//     partners of the packed SwiGLU / RoPE layouts (pack.py), so every epilogue is local to the wave;
//   * the wave walks K in 512-element steps: each lane streams 16 bytes of both W rows per step, two batches of four steps in
//     flight (16 x 16-byte loads per lane), the first batch requested before A is staged,
//     widens bf16 / fp16 to fp32 and accumulates M x 2 dot products in registers; a 6-step butterfly reduces across lanes;
//   * lane 0 applies bias / GELU / residual / SwiGLU / RoPE and stores.
// Algorithmic bytes per launch: N*K*2 (W) + M*K*2 (A) + outputs; the roofline is HBM (~6.3 TB/s achievable).
#include <cstdlib>
#include <type_traits>

#include "gemm_common.h"

namespace {
using namespace sg;

// VALU kernel: the weights are read exactly once per launch, in whole 128-byte lines per instruction: non-temporal loads (decode
// 3.23 -> 3.08 ms/token).  NOT in the matrix-core kernel, whose two loads per step touch the two halves of the same lines: there
// the hint costs the second half its cache hit (5 beams: 4.34 -> 4.66 ms).
__device__ __forceinline__ i32x4 ldw(const char* ptr) { return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(ptr)); }

template <typename T> __device__ __forceinline__ void widen8(i32x4 v, float* f);
template <> __device__ __forceinline__ void widen8<bf16_t>(i32x4 v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = __builtin_bit_cast(float, (uint32_t)v[e] << 16);
    f[2 * e + 1] = __builtin_bit_cast(float, (uint32_t)v[e] & 0xffff0000u);
  }
}
template <> __device__ __forceinline__ void widen8<f16_t>(i32x4 v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {   // (bit_cast<f16x2>(v[e]) mis-compiles here with ROCm 7.2: every e read element 0)
    const uint32_t u = (uint32_t)v[e];
    f[2 * e] = (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu));
    f[2 * e + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
  }
}

// epilogue of one output row for the column pair (c0, c1 = c0 + 32) — the [32 gate | 32 up] / [x_lo | x_hi] partners
// acc + a.lo * b.lo + a.hi * b.hi on packed 16-bit pairs (products are exact in fp32)
typedef __attribute__((ext_vector_type(2))) __bf16 gemv_bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 gemv_f16x2;
template <typename T> __device__ __forceinline__ float dot2_acc(int a, int b, float c);
template <> __device__ __forceinline__ float dot2_acc<bf16_t>(int a, int b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(gemv_bf16x2, a), __builtin_bit_cast(gemv_bf16x2, b), c, false);
}
template <> __device__ __forceinline__ float dot2_acc<f16_t>(int a, int b, float c) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(gemv_f16x2, a), __builtin_bit_cast(gemv_f16x2, b), c, false);
}

template <typename T, int EPI, int ACT, bool OF32>
__device__ __forceinline__ void gemv_store(const GemmParams& p, int m, int c0, int c1, float x, float y) {
  int64_t oo = (int64_t)m * p.ldo;
  if (p.o_rpb > 0) { const int bb = m / p.o_rpb; oo = (int64_t)bb * p.o_bs + (int64_t)(m - bb * p.o_rpb) * p.ldo; }
  if constexpr (EPI == STLLM_EPI_RESID) {
    float* o = reinterpret_cast<float*>(p.out) + oo;
    o[c0] = p.resid[(int64_t)m * p.ldr + c0] + x;
    o[c1] = p.resid[(int64_t)m * p.ldr + c1] + y;
  } else if constexpr (EPI == STLLM_EPI_SWIGLU) {
    store_elem<T>(p.out, oo + (c0 >> 6) * 32 + (c0 & 31), silu_f(x) * y);
  } else {
    if constexpr (EPI == STLLM_EPI_ROPE) {
      if (c0 < p.rope_cols) {
        const int fi = ((c0 >> 6) & 1) * 32 + (c0 & 31);
        const int pos = m % p.rope_seq;
        const float c = p.aux0[pos * 64 + fi], sn = p.aux1[pos * 64 + fi];
        const float xr = x * c - y * sn;
        y = y * c + x * sn;
        x = xr;
      }
    } else {
      if constexpr (ACT == STLLM_ACT_GELU) { x = gelu_erf(x); y = gelu_erf(y); }
      if constexpr (ACT == STLLM_ACT_RELU) { x = fmaxf(x, 0.0f); y = fmaxf(y, 0.0f); }
    }
    if constexpr (OF32 && EPI == STLLM_EPI_STORE) {
      float* o = reinterpret_cast<float*>(p.out) + oo;
      o[c0] = x;
      o[c1] = y;
    } else {
      store_elem<T>(p.out, oo + c0, x);
      store_elem<T>(p.out, oo + c1, y);
    }
  }
}

// Stage the MR rows of A (K x 2 bytes each; 2-level row indexing honoured) in LDS for a 256-thread workgroup; the caller's barrier follows.
// Shared by the 16-bit VALU kernel and its int8-weight twin (gemv_w8_kernel).
template <typename T, int MR>
__device__ __forceinline__ void gemv_stage_a(const GemmParams& p, char* smem, int tid, int lane, int wave) {
  const int K = p.K;
  const int row_bytes = K * 2;
  if (p.nx) {
    // A := RMSNorm(x) * gamma, computed here (Llama's input / post-attention norm fused into the projection of the decode step):
    // same arithmetic as norm_row_kernel<T, true> (variance in fp32 over the row, (x * rstd) * gamma, one rounding to T).  Every
    // workgroup recomputes it for the <= 8 rows — 16-32 KB of L2 reads against the weight panel it then streams from HBM.
    __shared__ float red[8];
    const int nvec = K >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(p.ngamma);
    for (int m = 0; m < MR; ++m) {
      const int gr = m < p.M ? m : p.M - 1;
      const float4* xr = reinterpret_cast<const float4*>(p.nx + (int64_t)gr * p.nx_ld);
      float ss = 0.0f;
      for (int c = tid; c < nvec; c += 256) {
        const float4 v = xr[c];
        ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      }
      ss = wave_sum(ss);
      if (lane == 0) red[(m & 1) * 4 + wave] = ss;      // two slots: row m + 1 may write while a slow wave still reads row m's
      __syncthreads();
      ss = red[(m & 1) * 4] + red[(m & 1) * 4 + 1] + red[(m & 1) * 4 + 2] + red[(m & 1) * 4 + 3];
      const float rstd = rsqrtf(ss / (float)K + p.neps);
      for (int c = tid; c < nvec; c += 256) {
        const float4 v = xr[c], g = g4[c];
        uint2 pk;
        pk.x = Elem<T>::pack2(v.x * rstd * g.x, v.y * rstd * g.y);
        pk.y = Elem<T>::pack2(v.z * rstd * g.z, v.w * rstd * g.w);
        *reinterpret_cast<uint2*>(smem + m * row_bytes + c * 8) = pk;
      }
    }
  } else {
    for (int m = 0; m < MR; ++m) {
      int gr = m < p.M ? m : p.M - 1;
      int64_t off = (int64_t)gr * p.lda_b;
      if (p.a_rpb > 0) { const int bb = gr / p.a_rpb; off = (int64_t)bb * p.a_bs_b + (int64_t)(gr - bb * p.a_rpb) * p.lda_b; }
      const char* src = p.A + off;
      for (int c = tid * 16; c < row_bytes; c += 256 * 16)
        *reinterpret_cast<i32x4*>(smem + m * row_bytes + c) = *reinterpret_cast<const i32x4*>(src + c);
    }
  }
}

template <typename T, int EPI, int ACT, bool OF32, int MR>
__global__ __launch_bounds__(256) void gemv_kernel(const GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // A: MR rows x K x 2 bytes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K;
  const int row_bytes = K * 2;
  // ---- this wave's column pair; its first kU steps of both W rows are requested BEFORE A is staged (the weight stream does not
  // depend on A: the HBM round trip overlaps the staging — and, with the fused RMSNorm operand, the two passes over x) -------------
  const int q = blockIdx.x * 4 + wave;           // column-pair index
  const int c0 = (q >> 5) * 64 + (q & 31), c1 = c0 + 32;
  const bool active = c0 < p.N;
  const char* w0 = p.W + (active ? (int64_t)c0 * p.ldw_b : 0);
  const char* w1 = p.W + (active ? (int64_t)c1 * p.ldw_b : 0);
  constexpr int kU = 4;                           // steps (1024 bytes of K per wave) per batch; two batches in flight
  const int lane_b = lane * 16;
  auto load_batch = [&](i32x4* wa, i32x4* wb, int kbase) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kb = kbase + u * 1024 + lane_b;
      if (kb < row_bytes) {
        wa[u] = ldw(w0 + kb);
        wb[u] = ldw(w1 + kb);
      }
    }
  };
  i32x4 wa0[kU], wb0[kU], wa1[kU], wb1[kU];
  load_batch(wa0, wb0, 0);
  gemv_stage_a<T, MR>(p, smem, tid, lane, wave);
  __syncthreads();

  if (!active) return;                            // (no barrier after this point)

  float acc[MR][2];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m][0] = acc[m][1] = 0.0f;

  // 8 elements of both W rows against the MR rows of A: v_dot2c_f32_{bf16,f16} multiplies two 16-bit pairs and adds them to an
  // fp32 accumulator in one instruction — no widening, 8 instructions per row instead of 24 (5 beams: the kernel is HBM-bound
  // again instead of VALU-bound)
  auto fma8 = [&](i32x4 wa, i32x4 wb, int kb) {   // kb = byte offset of this lane's 8 elements
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const i32x4 x = *reinterpret_cast<const i32x4*>(smem + m * row_bytes + kb);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[m][0] = dot2_acc<T>(x[e], wa[e], acc[m][0]);
        acc[m][1] = dot2_acc<T>(x[e], wb[e], acc[m][1]);
      }
    }
  };
  auto use_batch = [&](const i32x4* wa, const i32x4* wb, int kbase) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kb = kbase + u * 1024 + lane_b;
      if (kb < row_bytes) fma8(wa[u], wb[u], kb);   // ragged last step (K % 512 != 0): the lanes past the row end sit out
    }
  };
  // lane l owns bytes [l*16 + 1024*step, +16) of both W rows; two batches of kU steps (2 x 8 x 16-byte loads per lane) in flight
  for (int kbase = 0; kbase < row_bytes; kbase += 2 * kU * 1024) {
    load_batch(wa1, wb1, kbase + kU * 1024);
    use_batch(wa0, wb0, kbase);
    load_batch(wa0, wb0, kbase + 2 * kU * 1024);
    use_batch(wa1, wb1, kbase + kU * 1024);
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    acc[m][0] = wave_sum(acc[m][0]);
    acc[m][1] = wave_sum(acc[m][1]);
  }
  if (lane != 0) return;

  const float b0 = p.bias ? p.bias[c0] : 0.0f, b1 = p.bias ? p.bias[c1] : 0.0f;
  for (int m = 0; m < MR; ++m) {
    if (m >= p.M) break;
    gemv_store<T, EPI, ACT, OF32>(p, m, c0, c1, acc[m][0] + b0, acc[m][1] + b1);
  }
}

// ---- 3 <= M <= 16 rows: the same stream on the matrix cores -----------------------------------------------------------------------
// With more than two rows the VALU kernel above is bound by its own FMAs (5 beams: 160 VALU instructions per 2 KB of weights),
// not by HBM.  One v_mfma_f32_16x16x32 multiplies 16 rows of A with 32 k x 16 columns of W (1 KB of weights) in 8 cycles; rows
// M..15 are padding that costs nothing.
//   * a workgroup of 8 waves owns 16 columns — or, for the SwiGLU / RoPE epilogues, the 32 columns [c, c + 16) and [c + 32, c + 48)
//     of a 64-column group, so that every lane ends up with the (c, c + 32) partners of the packed layouts in two accumulators;
//   * lane l = (column n = l % 16, k-group g = l / 16) loads bytes [16 g, 16 g + 16) of both 64-byte halves of W row n's 128-byte
//     step: the four k-groups of a row cover one contiguous 64-byte sector per instruction, and the two MFMAs of a step take
//     k = [0, 32) and [32, 64) in natural order; A's rows are read with the same addressing;
//   * the 8 waves take every 8th 64-element k step (together 1 KB of every row per round); their partial sums meet in LDS and
//     wave 0 adds them in wave order (deterministic) and runs the epilogue.
constexpr int kGmWaves = 8;
template <typename T> __device__ __forceinline__ f32x4 mfma16(i32x4 a, i32x4 b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mfma16<bf16_t>(i32x4 a, i32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mfma16<f16_t>(i32x4 a, i32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// one output element of the column-local epilogues (STORE / RESID)
template <typename T, int EPI, int ACT, bool OF32>
__device__ __forceinline__ void gemv_store1(const GemmParams& p, int m, int c, float x) {
  int64_t oo = (int64_t)m * p.ldo;
  if (p.o_rpb > 0) { const int bb = m / p.o_rpb; oo = (int64_t)bb * p.o_bs + (int64_t)(m - bb * p.o_rpb) * p.ldo; }
  if constexpr (EPI == STLLM_EPI_RESID) {
    reinterpret_cast<float*>(p.out)[oo + c] = p.resid[(int64_t)m * p.ldr + c] + x;
  } else {
    if constexpr (ACT == STLLM_ACT_GELU) x = gelu_erf(x);
    if constexpr (ACT == STLLM_ACT_RELU) x = fmaxf(x, 0.0f);
    if constexpr (OF32) reinterpret_cast<float*>(p.out)[oo + c] = x;
    else store_elem<T>(p.out, oo + c, x);
  }
}

template <typename T, int EPI, int ACT, bool OF32>
__global__ __launch_bounds__(64 * kGmWaves, 4) void gemv_mfma_kernel(const GemmParams p) {
  // PAIR: the epilogue combines columns c and c + 32 (SwiGLU, RoPE) => the workgroup owns two 16-column blocks; otherwise ONE
  // block of 16 columns, which doubles the number of workgroups (o_proj / down_proj, N = 4096: 256 instead of 128 — one per CU)
  constexpr bool PAIR = (EPI == STLLM_EPI_SWIGLU || EPI == STLLM_EPI_ROPE);
  constexpr int NL = PAIR ? 6 : 4;              // 16-byte loads per lane and step
  __shared__ float red[kGmWaves * (PAIR ? 8 : 4) * 64];   // partial sums of the 8 waves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, g = lane >> 4;
  const int unit = blockIdx.x;
  const int col0 = PAIR ? (unit >> 1) * 64 + (unit & 1) * 16 + n16 : unit * 16 + n16, col1 = col0 + 32;
  const char* w0 = p.W + (int64_t)col0 * p.ldw_b + g * 16;
  const char* w1 = p.W + (int64_t)(PAIR ? col1 : col0) * p.ldw_b + g * 16;
  // A is NOT staged: the <= 16 rows (<= 350 KB, L2 / L1 resident) are read straight into the operand registers next to the weight
  // stream — no staging pass, no barrier before the first MFMA, no LDS footprint (K = 11008 with 8 or 16 rows fits as well).
  // Rows >= M of the 16-row operand: any valid row (their products land in output rows that are never stored).
  const int am = n16 < p.M ? n16 : p.M - 1;
  int64_t aoff = (int64_t)am * p.lda_b;
  if (p.a_rpb > 0) { const int bb = am / p.a_rpb; aoff = (int64_t)bb * p.a_bs_b + (int64_t)(am - bb * p.a_rpb) * p.lda_b; }
  const char* ax = p.A + aoff + g * 16;
  const int nsteps = p.K / 64;
  constexpr int U = 2;                           // steps per batch; two batches (2 x 2 NL x 16-byte loads per lane) in flight
  i32x4 wq[2][U][NL];
  // Steps past the end of K are NOT skipped (a load or an MFMA under a wave-uniform `if (st < nsteps)` was observed to read
  // stale registers on gfx950 whenever only part of a batch was valid — the waits the compiler counts for the full batch let
  // younger data slip): they re-read the last step and multiply it with a zeroed A operand instead.
  auto load_batch = [&](int b, int st0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int st = st0 + kGmWaves * u;
      st = st < nsteps ? st : nsteps - 1;
      wq[b][u][0] = *reinterpret_cast<const i32x4*>(ax + st * 128);
      wq[b][u][1] = *reinterpret_cast<const i32x4*>(ax + st * 128 + 64);
      wq[b][u][2] = *reinterpret_cast<const i32x4*>(w0 + st * 128);
      wq[b][u][3] = *reinterpret_cast<const i32x4*>(w0 + st * 128 + 64);
      if constexpr (PAIR) {
        wq[b][u][4] = *reinterpret_cast<const i32x4*>(w1 + st * 128);
        wq[b][u][5] = *reinterpret_cast<const i32x4*>(w1 + st * 128 + 64);
      }
    }
  };
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  auto use_batch = [&](int b, int st0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int keep = (st0 + kGmWaves * u < nsteps) ? -1 : 0;   // wave-uniform mask
      i32x4 x0 = wq[b][u][0], x1 = wq[b][u][1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { x0[e] &= keep; x1[e] &= keep; }
      acc0 = mfma16<T>(x0, wq[b][u][2], acc0);
      acc0 = mfma16<T>(x1, wq[b][u][3], acc0);
      if constexpr (PAIR) {
        acc1 = mfma16<T>(x0, wq[b][u][4], acc1);
        acc1 = mfma16<T>(x1, wq[b][u][5], acc1);
      }
    }
  };
  load_batch(0, wave);
  for (int st = wave; st < nsteps; st += 2 * U * kGmWaves) {
    load_batch(1, st + U * kGmWaves);
    use_batch(0, st);
    load_batch(0, st + 2 * U * kGmWaves);
    use_batch(1, st + U * kGmWaves);
  }
  constexpr int NR = PAIR ? 8 : 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[(wave * NR + r) * 64 + lane] = acc0[r];
    if constexpr (PAIR) red[(wave * NR + 4 + r) * 64 + lane] = acc1[r];
  }
  __syncthreads();
  if (wave != 0) return;
  const float b0 = p.bias ? p.bias[col0] : 0.0f, b1 = (PAIR && p.bias) ? p.bias[col1] : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * g + r;   // D register r of lane l is D[4 (l / 16) + r][l % 16]
    float x = 0.0f, y = 0.0f;
#pragma unroll
    for (int w = 0; w < kGmWaves; ++w) {
      x += red[(w * NR + r) * 64 + lane];
      if constexpr (PAIR) y += red[(w * NR + 4 + r) * 64 + lane];
    }
    if (m < p.M) {
      if constexpr (PAIR) gemv_store<T, EPI, ACT, OF32>(p, m, col0, col1, x + b0, y + b1);
      else gemv_store1<T, EPI, ACT, OF32>(p, m, col0, x + b0);
    }
  }
}

template <typename T, int EPI, int ACT, bool OF32>
int launch_gemv_mfma(const GemmParams& p, hipStream_t stream) {
  auto kern = gemv_mfma_kernel<T, EPI, ACT, OF32>;
  constexpr bool PAIR = (EPI == STLLM_EPI_SWIGLU || EPI == STLLM_EPI_ROPE);
  hipLaunchKernelGGL(kern, dim3(p.N / (PAIR ? 32 : 16)), dim3(64 * kGmWaves), 0, stream, p);
  STLLM_CHECK_LAUNCH("stllm_gemm(gemv_mfma)");
  {
    static const char* kEpi[] = {"STORE", "RESID", "SWIGLU", "ROPE", "PATCH"};
    static char name[96];
    static bool named = false;
    if (!named) {
      snprintf(name, sizeof(name), "gemv_mfma_kernel<%s,%s,%d,%d>", std::is_same<T, bf16_t>::value ? "bf16_t" : "f16_t", kEpi[EPI], ACT, (int)OF32);
      named = true;
    }
    stllm_set_last_kernel(name);
  }
  return STLLM_OK;
}

template <typename T>
int dispatch_gemv_mfma(int epilogue, const GemmParams& p, hipStream_t stream) {
  switch (epilogue) {
    case STLLM_EPI_STORE:
      if (p.act == STLLM_ACT_NONE) return p.out_is_f32 ? launch_gemv_mfma<T, STLLM_EPI_STORE, 0, true>(p, stream) : launch_gemv_mfma<T, STLLM_EPI_STORE, 0, false>(p, stream);
      if (p.act == STLLM_ACT_GELU && !p.out_is_f32) return launch_gemv_mfma<T, STLLM_EPI_STORE, 1, false>(p, stream);
      break;
    case STLLM_EPI_RESID: return launch_gemv_mfma<T, STLLM_EPI_RESID, 0, false>(p, stream);
    case STLLM_EPI_SWIGLU: return launch_gemv_mfma<T, STLLM_EPI_SWIGLU, 0, false>(p, stream);
    case STLLM_EPI_ROPE: return launch_gemv_mfma<T, STLLM_EPI_ROPE, 0, false>(p, stream);
  }
  return STLLM_ERR_UNSUPPORTED;
}

template <typename T, int EPI, int ACT, bool OF32, int MR>
int launch_gemv(const GemmParams& p, hipStream_t stream) {
  auto kern = gemv_kernel<T, EPI, ACT, OF32, MR>;
  const int lds = MR * p.K * 2;
  static StllmPerDevice lds_dev;   // largest dynamic-LDS size opted into, per device ordinal
  bool lds_first;
  const int lds_d = lds_dev.enter(&lds_first);
  if (lds_first || lds > lds_dev.value[lds_d]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return STLLM_ERR_UNSUPPORTED;
    lds_dev.value[lds_d] = lds;
    lds_dev.done(lds_d);
  }
  const int pairs = p.N / 2;
  hipLaunchKernelGGL(kern, dim3((pairs + 3) / 4), dim3(256), lds, stream, p);
  STLLM_CHECK_LAUNCH("stllm_gemm(gemv)");
  {
    static const char* kEpi[] = {"STORE", "RESID", "SWIGLU", "ROPE", "PATCH"};
    static char name[96];
    static bool named = false;
    if (!named) {
      snprintf(name, sizeof(name), "gemv_kernel<%s,%s,%d,%d,%d>", std::is_same<T, bf16_t>::value ? "bf16_t" : "f16_t", kEpi[EPI], ACT, (int)OF32, MR);
      named = true;
    }
    stllm_set_last_kernel(name);
  }
  return STLLM_OK;
}

template <typename T, int EPI, int ACT, bool OF32>
int launch_gemv_m(const GemmParams& p, hipStream_t stream) {
  switch (p.M) {
    case 1: return launch_gemv<T, EPI, ACT, OF32, 1>(p, stream);
    case 2: return launch_gemv<T, EPI, ACT, OF32, 2>(p, stream);
    case 3: case 4: return launch_gemv<T, EPI, ACT, OF32, 4>(p, stream);
    case 5: case 6: return launch_gemv<T, EPI, ACT, OF32, 6>(p, stream);
    default: return launch_gemv<T, EPI, ACT, OF32, 8>(p, stream);   // M = 7, 8
  }
}

template <typename T>
int dispatch_gemv(int epilogue, const GemmParams& p, hipStream_t stream) {
  switch (epilogue) {
    case STLLM_EPI_STORE:
      if (p.act == STLLM_ACT_NONE) return p.out_is_f32 ? launch_gemv_m<T, STLLM_EPI_STORE, 0, true>(p, stream) : launch_gemv_m<T, STLLM_EPI_STORE, 0, false>(p, stream);
      if (p.act == STLLM_ACT_GELU && !p.out_is_f32) return launch_gemv_m<T, STLLM_EPI_STORE, 1, false>(p, stream);
      break;
    case STLLM_EPI_RESID: return launch_gemv_m<T, STLLM_EPI_RESID, 0, false>(p, stream);
    case STLLM_EPI_SWIGLU: return launch_gemv_m<T, STLLM_EPI_SWIGLU, 0, false>(p, stream);
    case STLLM_EPI_ROPE: return launch_gemv_m<T, STLLM_EPI_ROPE, 0, false>(p, stream);
  }
  return STLLM_ERR_UNSUPPORTED;
}


// ---- W8A16: the same two kernels over int8 weights with one fp32 scale per output row (stllm_gemv_w8) -----------------------------
// The weight stream is half the bytes of the 16-bit kernels above; the integers (|q| <= 127, exact in bf16 and fp16) are widened to
// 16-bit pairs in registers and meet A on the same v_dot2c / v_mfma_f32_16x16x32 instructions, so the fp32 accumulators hold sums of
// exact products a * q.  scale[n] multiplies the finished sum once, in the epilogue, before bias / residual / SwiGLU / RoPE.
__device__ __forceinline__ uint32_t byte_perm(uint32_t s0, uint32_t s1, uint32_t sel) {   // v_perm_b32: selector 0-3 = bytes of s1, 4-7 = bytes of s0
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(s0, s1, sel);
#else
  const uint64_t v = ((uint64_t)s0 << 32) | s1;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) r |= (uint32_t)((v >> (8 * ((sel >> (8 * i)) & 7))) & 0xffu) << (8 * i);
  return r;
#endif
}
// four int8 of one dword -> two 16-bit pairs (lo = elements 0, 1; hi = elements 2, 3), exactly
template <typename T> __device__ __forceinline__ void cvt4(uint32_t w, int& lo, int& hi);
template <> __device__ __forceinline__ void cvt4<bf16_t>(uint32_t w, int& lo, int& hi) {
  // sign-extending byte -> fp32 conversions; an integer of magnitude <= 127 has 7 significant bits, so the upper half of its fp32 image IS its bf16 image
  const uint32_t f0 = __builtin_bit_cast(uint32_t, (float)(int8_t)(w & 0xffu)), f1 = __builtin_bit_cast(uint32_t, (float)(int8_t)((w >> 8) & 0xffu));
  const uint32_t f2 = __builtin_bit_cast(uint32_t, (float)(int8_t)((w >> 16) & 0xffu)), f3 = __builtin_bit_cast(uint32_t, (float)(int8_t)(w >> 24));
  lo = (int)byte_perm(f1, f0, 0x07060302u);
  hi = (int)byte_perm(f3, f2, 0x07060302u);
}
template <> __device__ __forceinline__ void cvt4<f16_t>(uint32_t w, int& lo, int& hi) {
  // magic number: fp16 0x6400 | u = 1024 + u has a unit of 1; with u = q + 128 (the byte with its sign bit flipped) 1024 + u - 1152 = q, exactly:
  // one xor per four weights, one v_perm_b32 and one v_pk_add_f16 per pair
  const uint32_t x = w ^ 0x80808080u;
  const gemv_f16x2 off = {(_Float16)1152.0f, (_Float16)1152.0f};
  lo = __builtin_bit_cast(int, __builtin_bit_cast(gemv_f16x2, byte_perm(0x64646464u, x, 0x04010400u)) - off);
  hi = __builtin_bit_cast(int, __builtin_bit_cast(gemv_f16x2, byte_perm(0x64646464u, x, 0x04030402u)) - off);
}
// 16 int8 -> eight 16-bit pairs in element order
template <typename T> __device__ __forceinline__ void cvt16(i32x4 w, int* pr) {
#pragma unroll
  for (int e = 0; e < 4; ++e) cvt4<T>((uint32_t)w[e], pr[2 * e], pr[2 * e + 1]);
}

// M <= 8 rows on the VALU: gemv_kernel's structure — a wave per column pair (c, c + 32), A staged in LDS behind the first batch of weight loads —
// with 16 weights per lane, row and step: a wave walks K in 1024-element steps (1 KiB of either W row)
template <typename T, int EPI, bool OF32, int MR>
__global__ __launch_bounds__(256) void gemv_w8_kernel(const GemmParams p, const float* __restrict__ scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // A: MR rows x K x 2 bytes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K;                              // = bytes of one W row
  const int a_row_bytes = K * 2;
  const int q = blockIdx.x * 4 + wave;           // column-pair index
  const int c0 = (q >> 5) * 64 + (q & 31), c1 = c0 + 32;
  const bool active = c0 < p.N;
  const char* w0 = p.W + (active ? (int64_t)c0 * p.ldw_b : 0);
  const char* w1 = p.W + (active ? (int64_t)c1 * p.ldw_b : 0);
  constexpr int kU = 4;                           // steps per batch; two batches (2 x 8 x 16-byte loads per lane) in flight
  const int lane_b = lane * 16;
  auto load_batch = [&](i32x4* wa, i32x4* wb, int kbase) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kb = kbase + u * 1024 + lane_b;
      if (kb < K) {
        wa[u] = ldw(w0 + kb);
        wb[u] = ldw(w1 + kb);
      }
    }
  };
  i32x4 wa0[kU], wb0[kU], wa1[kU], wb1[kU];
  load_batch(wa0, wb0, 0);                        // in flight before A is staged
  gemv_stage_a<T, MR>(p, smem, tid, lane, wave);
  __syncthreads();

  if (!active) return;                            // (no barrier after this point)

  float acc[MR][2];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m][0] = acc[m][1] = 0.0f;

  auto fma16 = [&](i32x4 wa, i32x4 wb, int kb) {   // kb = index of this lane's first of 16 elements
    int pa[8], pb[8];
    cvt16<T>(wa, pa);
    cvt16<T>(wb, pb);
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const i32x4 x0 = *reinterpret_cast<const i32x4*>(smem + m * a_row_bytes + kb * 2);
      const i32x4 x1 = *reinterpret_cast<const i32x4*>(smem + m * a_row_bytes + kb * 2 + 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[m][0] = dot2_acc<T>(x0[e], pa[e], acc[m][0]);
        acc[m][1] = dot2_acc<T>(x0[e], pb[e], acc[m][1]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[m][0] = dot2_acc<T>(x1[e], pa[4 + e], acc[m][0]);
        acc[m][1] = dot2_acc<T>(x1[e], pb[4 + e], acc[m][1]);
      }
    }
  };
  auto use_batch = [&](const i32x4* wa, const i32x4* wb, int kbase) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kb = kbase + u * 1024 + lane_b;
      if (kb < K) fma16(wa[u], wb[u], kb);        // ragged last step (K % 1024 != 0): the lanes past the row end sit out
    }
  };
  for (int kbase = 0; kbase < K; kbase += 2 * kU * 1024) {
    load_batch(wa1, wb1, kbase + kU * 1024);
    use_batch(wa0, wb0, kbase);
    load_batch(wa0, wb0, kbase + 2 * kU * 1024);
    use_batch(wa1, wb1, kbase + kU * 1024);
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    acc[m][0] = wave_sum(acc[m][0]);
    acc[m][1] = wave_sum(acc[m][1]);
  }
  if (lane != 0) return;

  const float s0 = scale[c0], s1 = scale[c1];
  const float b0 = p.bias ? p.bias[c0] : 0.0f, b1 = p.bias ? p.bias[c1] : 0.0f;
  for (int m = 0; m < MR; ++m) {
    if (m >= p.M) break;
    gemv_store<T, EPI, STLLM_ACT_NONE, OF32>(p, m, c0, c1, acc[m][0] * s0 + b0, acc[m][1] * s1 + b1);
  }
}

// 3 <= M <= 16 rows on the matrix cores: gemv_mfma_kernel's structure (8 waves per 16 columns, or per 2 x 16 partner columns; every wave takes
// every 8th 64-element k step; partial sums meet in LDS).  Lane l = (column n = l % 16, k-group g = l / 16) loads the 16 weights at bytes
// [16 g, 16 g + 16) of W row n's 64-byte step — the four k-groups of a row cover one contiguous 64-byte sector — and the 16 elements of A's row at
// bytes [32 g, 32 g + 32) of its 128-byte step; the two MFMAs of a step take the lower and the upper 8 of those 16.
template <typename T, int EPI, bool OF32>
__global__ __launch_bounds__(64 * kGmWaves, 4) void gemv_w8_mfma_kernel(const GemmParams p, const float* __restrict__ scale) {
  constexpr bool PAIR = (EPI == STLLM_EPI_SWIGLU || EPI == STLLM_EPI_ROPE);
  constexpr int NL = PAIR ? 4 : 3;              // 16-byte loads per lane and step: 2 of A, 1 or 2 of W
  __shared__ float red[kGmWaves * (PAIR ? 8 : 4) * 64];   // partial sums of the 8 waves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, g = lane >> 4;
  const int unit = blockIdx.x;
  const int col0 = PAIR ? (unit >> 1) * 64 + (unit & 1) * 16 + n16 : unit * 16 + n16, col1 = col0 + 32;
  const char* w0 = p.W + (int64_t)col0 * p.ldw_b + g * 16;
  const char* w1 = p.W + (int64_t)(PAIR ? col1 : col0) * p.ldw_b + g * 16;
  // A is read straight from global memory (L2 / L1 resident), as in gemv_mfma_kernel; rows >= M of the 16-row operand: any valid row
  const int am = n16 < p.M ? n16 : p.M - 1;
  int64_t aoff = (int64_t)am * p.lda_b;
  if (p.a_rpb > 0) { const int bb = am / p.a_rpb; aoff = (int64_t)bb * p.a_bs_b + (int64_t)(am - bb * p.a_rpb) * p.lda_b; }
  const char* ax = p.A + aoff + g * 32;
  const int nsteps = p.K / 64;
  constexpr int U = 2;                           // steps per batch; two batches in flight
  i32x4 wq[2][U][NL];
  // steps past the end of K re-read the last step and meet a zeroed A operand (see gemv_mfma_kernel: no partially valid batches)
  auto load_batch = [&](int b, int st0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int st = st0 + kGmWaves * u;
      st = st < nsteps ? st : nsteps - 1;
      wq[b][u][0] = *reinterpret_cast<const i32x4*>(ax + st * 128);
      wq[b][u][1] = *reinterpret_cast<const i32x4*>(ax + st * 128 + 16);
      wq[b][u][2] = *reinterpret_cast<const i32x4*>(w0 + st * 64);
      if constexpr (PAIR) wq[b][u][3] = *reinterpret_cast<const i32x4*>(w1 + st * 64);
    }
  };
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  auto use_batch = [&](int b, int st0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int keep = (st0 + kGmWaves * u < nsteps) ? -1 : 0;   // wave-uniform mask
      i32x4 x0 = wq[b][u][0], x1 = wq[b][u][1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { x0[e] &= keep; x1[e] &= keep; }
      int pr[8];
      cvt16<T>(wq[b][u][2], pr);
      acc0 = mfma16<T>(x0, i32x4{pr[0], pr[1], pr[2], pr[3]}, acc0);
      acc0 = mfma16<T>(x1, i32x4{pr[4], pr[5], pr[6], pr[7]}, acc0);
      if constexpr (PAIR) {
        cvt16<T>(wq[b][u][3], pr);
        acc1 = mfma16<T>(x0, i32x4{pr[0], pr[1], pr[2], pr[3]}, acc1);
        acc1 = mfma16<T>(x1, i32x4{pr[4], pr[5], pr[6], pr[7]}, acc1);
      }
    }
  };
  load_batch(0, wave);
  for (int st = wave; st < nsteps; st += 2 * U * kGmWaves) {
    load_batch(1, st + U * kGmWaves);
    use_batch(0, st);
    load_batch(0, st + 2 * U * kGmWaves);
    use_batch(1, st + U * kGmWaves);
  }
  constexpr int NR = PAIR ? 8 : 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[(wave * NR + r) * 64 + lane] = acc0[r];
    if constexpr (PAIR) red[(wave * NR + 4 + r) * 64 + lane] = acc1[r];
  }
  __syncthreads();
  if (wave != 0) return;
  const float s0 = scale[col0], s1 = PAIR ? scale[col1] : 0.0f;
  const float b0 = p.bias ? p.bias[col0] : 0.0f, b1 = (PAIR && p.bias) ? p.bias[col1] : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * g + r;   // D register r of lane l is D[4 (l / 16) + r][l % 16]
    float x = 0.0f, y = 0.0f;
#pragma unroll
    for (int w = 0; w < kGmWaves; ++w) {   // wave order: deterministic
      x += red[(w * NR + r) * 64 + lane];
      if constexpr (PAIR) y += red[(w * NR + 4 + r) * 64 + lane];
    }
    if (m < p.M) {
      if constexpr (PAIR) gemv_store<T, EPI, STLLM_ACT_NONE, OF32>(p, m, col0, col1, x * s0 + b0, y * s1 + b1);
      else gemv_store1<T, EPI, STLLM_ACT_NONE, OF32>(p, m, col0, x * s0 + b0);
    }
  }
}

const char* w8_kernel_name(char* buf, size_t cap, const char* family, bool bf16, int epi, bool of32, int mr) {
  static const char* kEpi[] = {"STORE", "RESID", "SWIGLU", "ROPE"};
  if (mr > 0) snprintf(buf, cap, "%s<%s,%s,%d,%d>", family, bf16 ? "bf16_t" : "f16_t", kEpi[epi], (int)of32, mr);
  else snprintf(buf, cap, "%s<%s,%s,%d>", family, bf16 ? "bf16_t" : "f16_t", kEpi[epi], (int)of32);
  return buf;
}

template <typename T, int EPI, bool OF32>
int launch_gemv_w8_mfma(const GemmParams& p, const float* scale, hipStream_t stream) {
  auto kern = gemv_w8_mfma_kernel<T, EPI, OF32>;
  constexpr bool PAIR = (EPI == STLLM_EPI_SWIGLU || EPI == STLLM_EPI_ROPE);
  hipLaunchKernelGGL(kern, dim3(p.N / (PAIR ? 32 : 16)), dim3(64 * kGmWaves), 0, stream, p, scale);
  STLLM_CHECK_LAUNCH("stllm_gemv_w8(mfma)");
  static char name[96];
  static const char* named = w8_kernel_name(name, sizeof(name), "gemv_w8_mfma_kernel", std::is_same<T, bf16_t>::value, EPI, OF32, 0);
  stllm_set_last_kernel(named);
  return STLLM_OK;
}

template <typename T, int EPI, bool OF32, int MR>
int launch_gemv_w8(const GemmParams& p, const float* scale, hipStream_t stream) {
  auto kern = gemv_w8_kernel<T, EPI, OF32, MR>;
  const int lds = MR * p.K * 2;
  static StllmPerDevice lds_dev;   // largest dynamic-LDS size opted into, per device ordinal
  bool lds_first;
  const int lds_d = lds_dev.enter(&lds_first);
  if (lds_first || lds > lds_dev.value[lds_d]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
      stllm_set_error("stllm_gemv_w8: cannot opt into %d bytes of LDS", lds);
      return STLLM_ERR_UNSUPPORTED;
    }
    lds_dev.value[lds_d] = lds;
    lds_dev.done(lds_d);
  }
  hipLaunchKernelGGL(kern, dim3((p.N / 2 + 3) / 4), dim3(256), lds, stream, p, scale);
  STLLM_CHECK_LAUNCH("stllm_gemv_w8(valu)");
  static char name[96];
  static const char* named = w8_kernel_name(name, sizeof(name), "gemv_w8_kernel", std::is_same<T, bf16_t>::value, EPI, OF32, MR);
  stllm_set_last_kernel(named);
  return STLLM_OK;
}

template <typename T, int EPI, bool OF32>
int launch_gemv_w8_any(const GemmParams& p, const float* scale, bool mfma, hipStream_t stream) {
  if (mfma) return launch_gemv_w8_mfma<T, EPI, OF32>(p, scale, stream);
  switch (p.M) {
    case 1: return launch_gemv_w8<T, EPI, OF32, 1>(p, scale, stream);
    case 2: return launch_gemv_w8<T, EPI, OF32, 2>(p, scale, stream);
    case 3: case 4: return launch_gemv_w8<T, EPI, OF32, 4>(p, scale, stream);
    case 5: case 6: return launch_gemv_w8<T, EPI, OF32, 6>(p, scale, stream);
    default: return launch_gemv_w8<T, EPI, OF32, 8>(p, scale, stream);   // M = 7, 8
  }
}

template <typename T>
int dispatch_gemv_w8(int epilogue, const GemmParams& p, const float* scale, bool mfma, hipStream_t stream) {
  switch (epilogue) {
    case STLLM_EPI_STORE:
      return p.out_is_f32 ? launch_gemv_w8_any<T, STLLM_EPI_STORE, true>(p, scale, mfma, stream) : launch_gemv_w8_any<T, STLLM_EPI_STORE, false>(p, scale, mfma, stream);
    case STLLM_EPI_RESID: return launch_gemv_w8_any<T, STLLM_EPI_RESID, false>(p, scale, mfma, stream);
    case STLLM_EPI_SWIGLU: return launch_gemv_w8_any<T, STLLM_EPI_SWIGLU, false>(p, scale, mfma, stream);
    default: return launch_gemv_w8_any<T, STLLM_EPI_ROPE, false>(p, scale, mfma, stream);
  }
}


// ---- W4A16 (q4): the same two kernels over 4-bit weights with one fp32 scale per output row and 128-element K group (stllm_gemv_q4) -------------
// A quarter of the 16-bit bytes.  Stored nibble u = q + 8 in [1, 15] (|q| <= 7).  Placement (pack.quant4_groups): of the 8 elements a dword holds,
// element 2 t sits at bits [4 t, 4 t + 4) and element 2 t + 1 at bits [16 + 4 t, 16 + 4 t + 4), so (w >> 4 t) & 0x000f000f is the K-adjacent pair t with
// one nibble at the bottom of either half: or-ing an exponent onto it makes a 16-bit float pair without moving a bit.
//   fp16: 0x6400 | u = 1024 + u, minus 1032 = q (one v_pk_add_f16).  The nibbles at bits [4, 8) need no shift either: 0x6400 | (u << 4) = 1024 + 16 u, and
//         (1024 + 16 u) / 16 - 72 = q exactly (one v_pk_fma_f16): one shift, four v_bfi_b32 and four packed ops per 8 weights.
//   bf16: 0x4300 | u = 128 + u is exact (8 significant bits), and gfx950's ISA lists no packed bf16 add: the pair meets A as it is, and the offset leaves in fp32,
//         partial - 136 sum(a), with sum(a) taken over the same elements by the same instruction against a pair of ones.
// The group sum is formed from zero and enters the accumulator as acc += scale[n, group] * partial, in fp32.
constexpr float kQ4Off = 136.0f;   // 128 + 8
// (a & mask) | (b & ~mask).  ASM: one v_bfi_b32.  Written as C++ with a constant b, hipcc (ROCm 7.2) folds b & ~mask and emits v_and_b32 + v_or_b32 with a
// literal each (a VOP3 v_and_or_b32 takes no literal on gfx9): 11 instead of 7 VALU instructions per 8 bf16 weights.  The asm form is for VALU consumers
// only (gemv_q4_kernel's v_dot2c): feeding a v_mfma straight from it gave garbage on the MI355X — the compiler does not see the asm's VGPR write when it
// places the wait states a matrix-core read of a fresh VALU result needs — so the matrix-core kernel, where the unpack is not the cost, keeps plain C++.
template <bool ASM> __device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (ASM) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(mask), "v"(a), "v"(b));
    return r;
  }
#endif
  return (a & mask) | (b & ~mask);
}
template <typename T> struct Q4;
template <> struct Q4<f16_t> {
  static constexpr bool kOffset = false;
  static constexpr int kOnes = 0x3c003c00;
  template <bool ASM> static __device__ __forceinline__ void cvt8(uint32_t w, int* pr) {   // 8 nibbles of one dword -> four pairs of q, in K order
    const gemv_f16x2 c0 = {(_Float16)1032.0f, (_Float16)1032.0f}, k1 = {(_Float16)0.0625f, (_Float16)0.0625f}, c1 = {(_Float16)72.0f, (_Float16)72.0f};
    const uint32_t h = w >> 8;
    pr[0] = __builtin_bit_cast(int, __builtin_bit_cast(gemv_f16x2, bfi<ASM>(0x000f000fu, w, 0x64006400u)) - c0);
    pr[1] = __builtin_bit_cast(int, __builtin_bit_cast(gemv_f16x2, bfi<ASM>(0x00f000f0u, w, 0x64006400u)) * k1 - c1);
    pr[2] = __builtin_bit_cast(int, __builtin_bit_cast(gemv_f16x2, bfi<ASM>(0x000f000fu, h, 0x64006400u)) - c0);
    pr[3] = __builtin_bit_cast(int, __builtin_bit_cast(gemv_f16x2, bfi<ASM>(0x00f000f0u, h, 0x64006400u)) * k1 - c1);
  }
};
template <> struct Q4<bf16_t> {
  static constexpr bool kOffset = true;
  static constexpr int kOnes = 0x3f803f80;
  template <bool ASM> static __device__ __forceinline__ void cvt8(uint32_t w, int* pr) {   // 8 nibbles of one dword -> four pairs of 128 + u = 136 + q, in K order
#pragma unroll
    for (int t = 0; t < 4; ++t) pr[t] = (int)bfi<ASM>(0x000f000fu, w >> (4 * t), 0x43004300u);
  }
};

// M <= 8 rows on the VALU: gemv_w8_kernel's structure with 32 weights per lane, row and 16-byte load: a wave walks K in 2048-element steps (1 KiB of
// either W row); a lane's 32 elements lie inside one scale group.  lds: leading dimension of scale (floats)
template <typename T, int EPI, bool OF32, int MR>
__global__ __launch_bounds__(256) void gemv_q4_kernel(const GemmParams p, const float* __restrict__ scale, const int lds) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // A: MR rows x K x 2 bytes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a_row_bytes = p.K * 2;
  const int w_row_bytes = p.K >> 1;
  const int q = blockIdx.x * 4 + wave;           // column-pair index
  const int c0 = (q >> 5) * 64 + (q & 31), c1 = c0 + 32;
  const bool active = c0 < p.N;
  const char* w0 = p.W + (active ? (int64_t)c0 * p.ldw_b : 0);
  const char* w1 = p.W + (active ? (int64_t)c1 * p.ldw_b : 0);
  const float* sc0 = scale + (active ? (int64_t)c0 * lds : 0);
  const float* sc1 = scale + (active ? (int64_t)c1 * lds : 0);
  constexpr int kU = 4;                           // steps per batch; two batches (2 x 8 x 16-byte loads per lane) in flight
  const int lane_b = lane * 16;
  auto load_batch = [&](i32x4* wa, i32x4* wb, float* sa, float* sb, int kbase) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kb = kbase + u * 1024 + lane_b;   // byte offset in the W row = element offset / 2; 64 bytes per scale group
      if (kb < w_row_bytes) {
        wa[u] = ldw(w0 + kb);
        wb[u] = ldw(w1 + kb);
        sa[u] = sc0[kb >> 6];
        sb[u] = sc1[kb >> 6];
      }
    }
  };
  i32x4 wa0[kU], wb0[kU], wa1[kU], wb1[kU];
  float sa0[kU], sb0[kU], sa1[kU], sb1[kU];
  load_batch(wa0, wb0, sa0, sb0, 0);              // in flight before A is staged
  gemv_stage_a<T, MR>(p, smem, tid, lane, wave);
  __syncthreads();

  if (!active) return;                            // (no barrier after this point)

  float acc[MR][2];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m][0] = acc[m][1] = 0.0f;

  auto fma32 = [&](i32x4 wa, i32x4 wb, float sa, float sb, int kb) {   // kb = byte offset of this lane's 16 bytes in the W row
    float t[MR][3];
#pragma unroll
    for (int m = 0; m < MR; ++m) t[m][0] = t[m][1] = t[m][2] = 0.0f;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      int pa[4], pb[4];
      Q4<T>::template cvt8<true>((uint32_t)wa[d], pa);
      Q4<T>::template cvt8<true>((uint32_t)wb[d], pb);
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const i32x4 x = *reinterpret_cast<const i32x4*>(smem + m * a_row_bytes + kb * 4 + d * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t[m][0] = dot2_acc<T>(x[e], pa[e], t[m][0]);
          t[m][1] = dot2_acc<T>(x[e], pb[e], t[m][1]);
          if constexpr (Q4<T>::kOffset) t[m][2] = dot2_acc<T>(x[e], Q4<T>::kOnes, t[m][2]);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      if constexpr (Q4<T>::kOffset) { t[m][0] -= kQ4Off * t[m][2]; t[m][1] -= kQ4Off * t[m][2]; }
      acc[m][0] += sa * t[m][0];
      acc[m][1] += sb * t[m][1];
    }
  };
  auto use_batch = [&](const i32x4* wa, const i32x4* wb, const float* sa, const float* sb, int kbase) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kb = kbase + u * 1024 + lane_b;
      if (kb < w_row_bytes) fma32(wa[u], wb[u], sa[u], sb[u], kb);   // ragged last step (K % 2048 != 0): the lanes past the row end sit out
    }
  };
  for (int kbase = 0; kbase < w_row_bytes; kbase += 2 * kU * 1024) {
    load_batch(wa1, wb1, sa1, sb1, kbase + kU * 1024);
    use_batch(wa0, wb0, sa0, sb0, kbase);
    load_batch(wa0, wb0, sa0, sb0, kbase + 2 * kU * 1024);
    use_batch(wa1, wb1, sa1, sb1, kbase + kU * 1024);
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    acc[m][0] = wave_sum(acc[m][0]);
    acc[m][1] = wave_sum(acc[m][1]);
  }
  if (lane != 0) return;

  const float b0 = p.bias ? p.bias[c0] : 0.0f, b1 = p.bias ? p.bias[c1] : 0.0f;
  for (int m = 0; m < MR; ++m) {
    if (m >= p.M) break;
    gemv_store<T, EPI, STLLM_ACT_NONE, OF32>(p, m, c0, c1, acc[m][0] + b0, acc[m][1] + b1);
  }
}

// 3 <= M <= 16 rows on the matrix cores: gemv_w8_mfma_kernel's structure (8 waves per 16 columns, or per 2 x 16 partner columns; partial sums meet in
// LDS in wave order) with a step of 128 K elements = one scale group.  Lane l = (column n = l % 16, k-group g = l / 16) loads the 32 weights at bytes
// [16 g, 16 g + 16) of W row n's 64-byte step and the same 32 elements of A's row n (bytes [64 g, 64 g + 64) of its 256-byte step); MFMA j of the four
// takes dword j of the weights (8 elements) against the j-th 16 bytes of A.  The four accumulate into a zeroed temporary; D register r of lane l
// belongs to column l % 16, so acc += scale[column, step] * tmp is a per-lane scalar multiply.  bf16: a fifth..eighth MFMA against a B operand of
// ones puts sum(a) of the step into the same D layout, and 136 sum(a) leaves tmp in fp32 (see Q4).
template <typename T, int EPI, bool OF32>
__global__ __launch_bounds__(64 * kGmWaves, 4) void gemv_q4_mfma_kernel(const GemmParams p, const float* __restrict__ scale, const int lds) {
  constexpr bool PAIR = (EPI == STLLM_EPI_SWIGLU || EPI == STLLM_EPI_ROPE);
  constexpr int NW = PAIR ? 2 : 1;              // 16-byte weight loads per lane and step (next to 4 of A)
  __shared__ float red[kGmWaves * (PAIR ? 8 : 4) * 64];   // partial sums of the 8 waves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, g = lane >> 4;
  const int unit = blockIdx.x;
  const int col0 = PAIR ? (unit >> 1) * 64 + (unit & 1) * 16 + n16 : unit * 16 + n16, col1 = col0 + 32;
  const char* w0 = p.W + (int64_t)col0 * p.ldw_b + g * 16;
  const char* w1 = p.W + (int64_t)(PAIR ? col1 : col0) * p.ldw_b + g * 16;
  const float* sc0 = scale + (int64_t)col0 * lds;
  const float* sc1 = scale + (int64_t)(PAIR ? col1 : col0) * lds;
  // A is read straight from global memory (L2 / L1 resident), as in gemv_mfma_kernel; rows >= M of the 16-row operand: any valid row
  const int am = n16 < p.M ? n16 : p.M - 1;
  int64_t aoff = (int64_t)am * p.lda_b;
  if (p.a_rpb > 0) { const int bb = am / p.a_rpb; aoff = (int64_t)bb * p.a_bs_b + (int64_t)(am - bb * p.a_rpb) * p.lda_b; }
  const char* ax = p.A + aoff + g * 64;
  const int nsteps = p.K / 128;
  i32x4 xq[2][4], wq[2][NW];                     // one step per batch; two batches in flight
  float sq[2][NW];
  // steps past the end of K re-read the last step and meet a zeroed A operand (see gemv_mfma_kernel: no partially valid batches)
  auto load_batch = [&](int b, int st) {
    st = st < nsteps ? st : nsteps - 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) xq[b][j] = *reinterpret_cast<const i32x4*>(ax + st * 256 + j * 16);
    wq[b][0] = *reinterpret_cast<const i32x4*>(w0 + st * 64);
    sq[b][0] = sc0[st];
    if constexpr (PAIR) {
      wq[b][1] = *reinterpret_cast<const i32x4*>(w1 + st * 64);
      sq[b][1] = sc1[st];
    }
  };
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const i32x4 ones = {Q4<T>::kOnes, Q4<T>::kOnes, Q4<T>::kOnes, Q4<T>::kOnes};
  auto use_batch = [&](int b, int st) {
    const int keep = (st < nsteps) ? -1 : 0;   // wave-uniform mask
    f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f}, ts = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      i32x4 x = xq[b][j];
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] &= keep;
      int pr[4];
      Q4<T>::template cvt8<false>((uint32_t)wq[b][0][j], pr);
      t0 = mfma16<T>(x, i32x4{pr[0], pr[1], pr[2], pr[3]}, t0);
      if constexpr (PAIR) {
        Q4<T>::template cvt8<false>((uint32_t)wq[b][1][j], pr);
        t1 = mfma16<T>(x, i32x4{pr[0], pr[1], pr[2], pr[3]}, t1);
      }
      if constexpr (Q4<T>::kOffset) ts = mfma16<T>(x, ones, ts);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (Q4<T>::kOffset) { t0[r] -= kQ4Off * ts[r]; t1[r] -= kQ4Off * ts[r]; }
      acc0[r] += sq[b][0] * t0[r];
      if constexpr (PAIR) acc1[r] += sq[b][1] * t1[r];
    }
  };
  load_batch(0, wave);
  for (int st = wave; st < nsteps; st += 2 * kGmWaves) {
    load_batch(1, st + kGmWaves);
    use_batch(0, st);
    load_batch(0, st + 2 * kGmWaves);
    use_batch(1, st + kGmWaves);
  }
  constexpr int NR = PAIR ? 8 : 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[(wave * NR + r) * 64 + lane] = acc0[r];
    if constexpr (PAIR) red[(wave * NR + 4 + r) * 64 + lane] = acc1[r];
  }
  __syncthreads();
  if (wave != 0) return;
  const float b0 = p.bias ? p.bias[col0] : 0.0f, b1 = (PAIR && p.bias) ? p.bias[col1] : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * g + r;   // D register r of lane l is D[4 (l / 16) + r][l % 16]
    float x = 0.0f, y = 0.0f;
#pragma unroll
    for (int w = 0; w < kGmWaves; ++w) {   // wave order: deterministic
      x += red[(w * NR + r) * 64 + lane];
      if constexpr (PAIR) y += red[(w * NR + 4 + r) * 64 + lane];
    }
    if (m < p.M) {
      if constexpr (PAIR) gemv_store<T, EPI, STLLM_ACT_NONE, OF32>(p, m, col0, col1, x + b0, y + b1);
      else gemv_store1<T, EPI, STLLM_ACT_NONE, OF32>(p, m, col0, x + b0);
    }
  }
}

template <typename T, int EPI, bool OF32>
int launch_gemv_q4_mfma(const GemmParams& p, const float* scale, int lds, hipStream_t stream) {
  auto kern = gemv_q4_mfma_kernel<T, EPI, OF32>;
  constexpr bool PAIR = (EPI == STLLM_EPI_SWIGLU || EPI == STLLM_EPI_ROPE);
  hipLaunchKernelGGL(kern, dim3(p.N / (PAIR ? 32 : 16)), dim3(64 * kGmWaves), 0, stream, p, scale, lds);
  STLLM_CHECK_LAUNCH("stllm_gemv_q4(mfma)");
  static char name[96];
  static const char* named = w8_kernel_name(name, sizeof(name), "gemv_q4_mfma_kernel", std::is_same<T, bf16_t>::value, EPI, OF32, 0);
  stllm_set_last_kernel(named);
  return STLLM_OK;
}

template <typename T, int EPI, bool OF32, int MR>
int launch_gemv_q4(const GemmParams& p, const float* scale, int lds, hipStream_t stream) {
  auto kern = gemv_q4_kernel<T, EPI, OF32, MR>;
  const int smem = MR * p.K * 2;
  static StllmPerDevice lds_dev;   // largest dynamic-LDS size opted into, per device ordinal
  bool lds_first;
  const int lds_d = lds_dev.enter(&lds_first);
  if (lds_first || smem > lds_dev.value[lds_d]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) {
      stllm_set_error("stllm_gemv_q4: cannot opt into %d bytes of LDS", smem);
      return STLLM_ERR_UNSUPPORTED;
    }
    lds_dev.value[lds_d] = smem;
    lds_dev.done(lds_d);
  }
  hipLaunchKernelGGL(kern, dim3((p.N / 2 + 3) / 4), dim3(256), smem, stream, p, scale, lds);
  STLLM_CHECK_LAUNCH("stllm_gemv_q4(valu)");
  static char name[96];
  static const char* named = w8_kernel_name(name, sizeof(name), "gemv_q4_kernel", std::is_same<T, bf16_t>::value, EPI, OF32, MR);
  stllm_set_last_kernel(named);
  return STLLM_OK;
}

template <typename T, int EPI, bool OF32>
int launch_gemv_q4_any(const GemmParams& p, const float* scale, int lds, bool mfma, hipStream_t stream) {
  if (mfma) return launch_gemv_q4_mfma<T, EPI, OF32>(p, scale, lds, stream);
  switch (p.M) {
    case 1: return launch_gemv_q4<T, EPI, OF32, 1>(p, scale, lds, stream);
    case 2: return launch_gemv_q4<T, EPI, OF32, 2>(p, scale, lds, stream);
    case 3: case 4: return launch_gemv_q4<T, EPI, OF32, 4>(p, scale, lds, stream);
    case 5: case 6: return launch_gemv_q4<T, EPI, OF32, 6>(p, scale, lds, stream);
    default: return launch_gemv_q4<T, EPI, OF32, 8>(p, scale, lds, stream);   // M = 7, 8
  }
}

template <typename T>
int dispatch_gemv_q4(int epilogue, const GemmParams& p, const float* scale, int lds, bool mfma, hipStream_t stream) {
  switch (epilogue) {
    case STLLM_EPI_STORE:
      return p.out_is_f32 ? launch_gemv_q4_any<T, STLLM_EPI_STORE, true>(p, scale, lds, mfma, stream) : launch_gemv_q4_any<T, STLLM_EPI_STORE, false>(p, scale, lds, mfma, stream);
    case STLLM_EPI_RESID: return launch_gemv_q4_any<T, STLLM_EPI_RESID, false>(p, scale, lds, mfma, stream);
    case STLLM_EPI_SWIGLU: return launch_gemv_q4_any<T, STLLM_EPI_SWIGLU, false>(p, scale, lds, mfma, stream);
    default: return launch_gemv_q4_any<T, STLLM_EPI_ROPE, false>(p, scale, lds, mfma, stream);
  }
}

}  // namespace

// M <= 16 (the caller decides how far it goes), 16-bit dtypes.  M >= 3 (option "gemv_mfma": 0 never, 1 from M = 1): the matrix-core
// kernel (K % 64 == 0; A is read straight from global memory, no LDS limit); otherwise, for M <= 8, the VALU kernel,
// whose staged rows (1, 2, 4, 6 or 8 x K x 2 bytes) must fit the LDS.  Returns STLLM_ERR_UNSUPPORTED when neither applies (the caller
// falls back to the tile kernels).
int stllm_gemv_launch(int dtype, int epilogue, const sg::GemmParams& p, hipStream_t stream) {
  if (p.M < 1 || p.M > 16) return STLLM_ERR_UNSUPPORTED;
  if (p.N % 64 || p.K % 8 || (p.ldw_b % 16) || (!p.nx && (p.lda_b % 16))) return STLLM_ERR_UNSUPPORTED;
  const int g_gemv_mfma = stllm_options().gemv_mfma;
  const int from = g_gemv_mfma == 0 ? 17 : g_gemv_mfma >= 1 ? g_gemv_mfma : 3;   // n >= 1: from M = n
  if (!p.nx && p.M >= from && p.K % 64 == 0) {
    if (dtype == STLLM_BF16) return dispatch_gemv_mfma<bf16_t>(epilogue, p, stream);
    if (dtype == STLLM_F16) return dispatch_gemv_mfma<f16_t>(epilogue, p, stream);
    return STLLM_ERR_UNSUPPORTED;
  }
  if (p.M > 8) return STLLM_ERR_UNSUPPORTED;
  const int mr = p.M <= 2 ? p.M : (p.M + 1) / 2 * 2;
  if ((int64_t)mr * p.K * 2 > 150 * 1024) return STLLM_ERR_UNSUPPORTED;
  if (p.nx && (p.K % 4 || p.nx_ld % 4 || p.a_rpb > 0)) return STLLM_ERR_UNSUPPORTED;
  if (dtype == STLLM_BF16) return dispatch_gemv<bf16_t>(epilogue, p, stream);
  if (dtype == STLLM_F16) return dispatch_gemv<f16_t>(epilogue, p, stream);
  return STLLM_ERR_UNSUPPORTED;
}

int stllm_prof_begin(const stllm_gemm_args* a, void* stream);     // profile.cpp
void stllm_prof_end(int idx, int rc, const stllm_gemm_args* a, void* stream);

// W8A16 entry point (include/stllm_hip.h).  No fallback: what neither kernel covers is STLLM_ERR_UNSUPPORTED with a message.
extern "C" int stllm_gemv_w8(const stllm_gemv_w8_args* a, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(a != nullptr, "stllm_gemv_w8: null args");
  if (a->dtype != STLLM_BF16 && a->dtype != STLLM_F16) {
    stllm_set_error("stllm_gemv_w8: A must be bf16 or fp16 (dtype %d)", a->dtype);
    return STLLM_ERR_BAD_DTYPE;
  }
  STLLM_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "stllm_gemv_w8: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
  STLLM_CHECK_ARG(a->N % 64 == 0 && a->K % 16 == 0, "stllm_gemv_w8: need N %% 64 == 0 and K %% 16 == 0 (N=%d K=%d)", a->N, a->K);
  STLLM_CHECK_ARG(a->Wq && aligned16(a->Wq) && a->ldw % 16 == 0 && a->ldw >= a->K, "stllm_gemv_w8: Wq null / not 16-byte aligned, or bad ldw %lld", (long long)a->ldw);
  STLLM_CHECK_ARG(a->scale != nullptr, "stllm_gemv_w8: scale is null");
  if (a->a_norm_x) {
    STLLM_CHECK_ARG(a->a_norm_gamma && aligned16(a->a_norm_x) && aligned16(a->a_norm_gamma) && a->a_norm_ldx >= a->K && a->a_norm_ldx % 4 == 0 && a->a_rows_per_batch == 0,
                    "stllm_gemv_w8(a_norm): the fused RMSNorm operand needs flat 16-byte aligned fp32 rows and gamma (M=%d)", a->M);
  } else {
    STLLM_CHECK_ARG(a->A && aligned16(a->A) && (a->lda * 2) % 16 == 0 && a->lda >= a->K && (a->a_batch_stride * 2) % 16 == 0,
                    "stllm_gemv_w8: A null / not 16-byte aligned, or bad lda %lld", (long long)a->lda);
  }
  STLLM_CHECK_ARG(a->out != nullptr && aligned16(a->out), "stllm_gemv_w8: out null or not 16-byte aligned");
  if (a->epilogue < STLLM_EPI_STORE || a->epilogue > STLLM_EPI_ROPE) {
    stllm_set_error("stllm_gemv_w8: epilogue %d is not one of STORE / RESID / SWIGLU / ROPE", a->epilogue);
    return STLLM_ERR_UNSUPPORTED;
  }
  {
    const bool f32o = a->epilogue == STLLM_EPI_RESID || (a->epilogue == STLLM_EPI_STORE && a->out_is_f32);
    const int oes = f32o ? 4 : 2;
    STLLM_CHECK_ARG((a->ldo * oes) % 16 == 0 && (a->o_batch_stride * oes) % 16 == 0,
                    "stllm_gemv_w8: output row/batch stride must be a multiple of 16 bytes (ldo=%lld)", (long long)a->ldo);
  }
  if (a->epilogue == STLLM_EPI_RESID)
    STLLM_CHECK_ARG(a->resid != nullptr && aligned16(a->resid) && a->ldr % 4 == 0, "stllm_gemv_w8(RESID): resid null / misaligned");
  if (a->epilogue == STLLM_EPI_ROPE)
    STLLM_CHECK_ARG(a->rope_cos && a->rope_sin && a->rope_seq > 0 && a->rope_cols % 128 == 0, "stllm_gemv_w8(ROPE): need cos/sin tables, rope_seq, rope_cols%%128==0");
  if (a->M > 16) {
    stllm_set_error("stllm_gemv_w8: M=%d is outside the decode regime (M <= 16)", a->M);
    return STLLM_ERR_UNSUPPORTED;
  }
  if (a->a_norm_x && a->M > 2) {
    stllm_set_error("stllm_gemv_w8(a_norm): no kernel for M=%d with the fused RMSNorm operand (M <= 2): run stllm_rmsnorm first", a->M);
    return STLLM_ERR_UNSUPPORTED;
  }
  const int g_gemv_mfma = stllm_options().gemv_mfma;
  const int from = g_gemv_mfma == 0 ? 17 : g_gemv_mfma >= 1 ? g_gemv_mfma : 3;   // n >= 1: from M = n
  const bool mfma = !a->a_norm_x && a->M >= from && a->K % 64 == 0;
  if (!mfma) {   // the VALU kernel: its staged rows must fit the LDS
    const int mr = a->M <= 2 ? a->M : (a->M + 1) / 2 * 2;
    if (a->M > 8 || (int64_t)mr * a->K * 2 > 150 * 1024) {
      stllm_set_error("stllm_gemv_w8: no kernel for M=%d K=%d%s (matrix-core kernel: K %% 64 == 0, no a_norm, option gemv_mfma=%d; VALU kernel: M <= 8 and %d x K x 2 bytes <= 150 KiB)",
                      a->M, a->K, a->a_norm_x ? " with a_norm" : "", g_gemv_mfma, mr);
      return STLLM_ERR_UNSUPPORTED;
    }
  }
  sg::GemmParams p{};
  p.A = reinterpret_cast<const char*>(a->A); p.lda_b = a->lda * 2;
  p.W = reinterpret_cast<const char*>(a->Wq); p.ldw_b = a->ldw;
  p.bias = a->bias; p.out = a->out; p.ldo = a->ldo; p.resid = a->resid; p.ldr = a->ldr;
  p.aux0 = a->rope_cos; p.aux1 = a->rope_sin; p.rope_seq = a->rope_seq; p.rope_cols = a->rope_cols;
  p.M = a->M; p.N = a->N; p.K = a->K; p.act = STLLM_ACT_NONE; p.out_is_f32 = a->out_is_f32;
  p.nx = a->a_norm_x; p.nx_ld = a->a_norm_ldx; p.ngamma = a->a_norm_gamma; p.neps = a->a_norm_eps;
  p.a_rpb = a->a_rows_per_batch; p.a_bs_b = a->a_batch_stride * 2;
  p.o_rpb = a->o_rows_per_batch; p.o_bs = a->o_batch_stride;
  stllm_gemm_args key{};   // what stllm_gemm_profile keys and reports a launch by; dtype + 16 keeps the int8 launches apart from 16-bit ones of the same shape
  key.dtype = a->dtype + 16; key.epilogue = a->epilogue; key.out_is_f32 = a->out_is_f32; key.M = a->M; key.N = a->N; key.K = a->K;
  const int prof_rec = stllm_prof_begin(&key, stream_);
  const int rc = a->dtype == STLLM_BF16 ? dispatch_gemv_w8<bf16_t>(a->epilogue, p, a->scale, mfma, stream)
                                        : dispatch_gemv_w8<f16_t>(a->epilogue, p, a->scale, mfma, stream);
  stllm_prof_end(prof_rec, rc, &key, stream_);
  return rc;
}

// W4A16 entry point (include/stllm_hip.h).  No fallback: what neither kernel covers is STLLM_ERR_UNSUPPORTED with a message.
extern "C" int stllm_gemv_q4(const stllm_gemv_q4_args* a, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  STLLM_CHECK_ARG(a != nullptr, "stllm_gemv_q4: null args");
  if (a->dtype != STLLM_BF16 && a->dtype != STLLM_F16) {
    stllm_set_error("stllm_gemv_q4: A must be bf16 or fp16 (dtype %d)", a->dtype);
    return STLLM_ERR_BAD_DTYPE;
  }
  STLLM_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "stllm_gemv_q4: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
  STLLM_CHECK_ARG(a->N % 64 == 0 && a->K % 128 == 0, "stllm_gemv_q4: need N %% 64 == 0 and K %% 128 == 0 (N=%d K=%d)", a->N, a->K);
  STLLM_CHECK_ARG(a->Wq && aligned16(a->Wq) && a->ldw % 16 == 0 && a->ldw >= a->K / 2, "stllm_gemv_q4: Wq null / not 16-byte aligned, or bad ldw %lld", (long long)a->ldw);
  STLLM_CHECK_ARG(a->scale != nullptr && a->ld_scale >= a->K / 128 && a->ld_scale <= 0x7fffffff, "stllm_gemv_q4: scale is null, or bad ld_scale %lld", (long long)a->ld_scale);
  if (a->a_norm_x) {
    STLLM_CHECK_ARG(a->a_norm_gamma && aligned16(a->a_norm_x) && aligned16(a->a_norm_gamma) && a->a_norm_ldx >= a->K && a->a_norm_ldx % 4 == 0 && a->a_rows_per_batch == 0,
                    "stllm_gemv_q4(a_norm): the fused RMSNorm operand needs flat 16-byte aligned fp32 rows and gamma (M=%d)", a->M);
  } else {
    STLLM_CHECK_ARG(a->A && aligned16(a->A) && (a->lda * 2) % 16 == 0 && a->lda >= a->K && (a->a_batch_stride * 2) % 16 == 0,
                    "stllm_gemv_q4: A null / not 16-byte aligned, or bad lda %lld", (long long)a->lda);
  }
  STLLM_CHECK_ARG(a->out != nullptr && aligned16(a->out), "stllm_gemv_q4: out null or not 16-byte aligned");
  if (a->epilogue < STLLM_EPI_STORE || a->epilogue > STLLM_EPI_ROPE) {
    stllm_set_error("stllm_gemv_q4: epilogue %d is not one of STORE / RESID / SWIGLU / ROPE", a->epilogue);
    return STLLM_ERR_UNSUPPORTED;
  }
  {
    const bool f32o = a->epilogue == STLLM_EPI_RESID || (a->epilogue == STLLM_EPI_STORE && a->out_is_f32);
    const int oes = f32o ? 4 : 2;
    STLLM_CHECK_ARG((a->ldo * oes) % 16 == 0 && (a->o_batch_stride * oes) % 16 == 0,
                    "stllm_gemv_q4: output row/batch stride must be a multiple of 16 bytes (ldo=%lld)", (long long)a->ldo);
  }
  if (a->epilogue == STLLM_EPI_RESID)
    STLLM_CHECK_ARG(a->resid != nullptr && aligned16(a->resid) && a->ldr % 4 == 0, "stllm_gemv_q4(RESID): resid null / misaligned");
  if (a->epilogue == STLLM_EPI_ROPE)
    STLLM_CHECK_ARG(a->rope_cos && a->rope_sin && a->rope_seq > 0 && a->rope_cols % 128 == 0, "stllm_gemv_q4(ROPE): need cos/sin tables, rope_seq, rope_cols%%128==0");
  if (a->M > 16) {
    stllm_set_error("stllm_gemv_q4: M=%d is outside the decode regime (M <= 16)", a->M);
    return STLLM_ERR_UNSUPPORTED;
  }
  if (a->a_norm_x && a->M > 2) {
    stllm_set_error("stllm_gemv_q4(a_norm): no kernel for M=%d with the fused RMSNorm operand (M <= 2): run stllm_rmsnorm first", a->M);
    return STLLM_ERR_UNSUPPORTED;
  }
  const int g_gemv_mfma = stllm_options().gemv_mfma;
  const int from = g_gemv_mfma == 0 ? 17 : g_gemv_mfma >= 1 ? g_gemv_mfma : 3;   // n >= 1: from M = n
  const bool mfma = !a->a_norm_x && a->M >= from;   // (K % 128 == 0 always holds here)
  if (!mfma) {   // the VALU kernel: its staged rows must fit the LDS
    const int mr = a->M <= 2 ? a->M : (a->M + 1) / 2 * 2;
    if (a->M > 8 || (int64_t)mr * a->K * 2 > 150 * 1024) {
      stllm_set_error("stllm_gemv_q4: no kernel for M=%d K=%d%s (matrix-core kernel: no a_norm, option gemv_mfma=%d; VALU kernel: M <= 8 and %d x K x 2 bytes <= 150 KiB)",
                      a->M, a->K, a->a_norm_x ? " with a_norm" : "", g_gemv_mfma, mr);
      return STLLM_ERR_UNSUPPORTED;
    }
  }
  sg::GemmParams p{};
  p.A = reinterpret_cast<const char*>(a->A); p.lda_b = a->lda * 2;
  p.W = reinterpret_cast<const char*>(a->Wq); p.ldw_b = a->ldw;
  p.bias = a->bias; p.out = a->out; p.ldo = a->ldo; p.resid = a->resid; p.ldr = a->ldr;
  p.aux0 = a->rope_cos; p.aux1 = a->rope_sin; p.rope_seq = a->rope_seq; p.rope_cols = a->rope_cols;
  p.M = a->M; p.N = a->N; p.K = a->K; p.act = STLLM_ACT_NONE; p.out_is_f32 = a->out_is_f32;
  p.nx = a->a_norm_x; p.nx_ld = a->a_norm_ldx; p.ngamma = a->a_norm_gamma; p.neps = a->a_norm_eps;
  p.a_rpb = a->a_rows_per_batch; p.a_bs_b = a->a_batch_stride * 2;
  p.o_rpb = a->o_rows_per_batch; p.o_bs = a->o_batch_stride;
  stllm_gemm_args key{};   // what stllm_gemm_profile keys and reports a launch by; dtype + 32 keeps the 4-bit launches apart from the 16-bit (+ 0) and int8 (+ 16) ones of the same shape
  key.dtype = a->dtype + 32; key.epilogue = a->epilogue; key.out_is_f32 = a->out_is_f32; key.M = a->M; key.N = a->N; key.K = a->K;
  const int prof_rec = stllm_prof_begin(&key, stream_);
  const int lds = (int)a->ld_scale;
  const int rc = a->dtype == STLLM_BF16 ? dispatch_gemv_q4<bf16_t>(a->epilogue, p, a->scale, lds, mfma, stream)
                                        : dispatch_gemv_q4<f16_t>(a->epilogue, p, a->scale, lds, mfma, stream);
  stllm_prof_end(prof_rec, rc, &key, stream_);
  return rc;
}
