// LoRA down projection (peft Linear: lora_A of q_proj and v_proj stacked to one [2 r, K] weight): t = x · Aᵀ, [M, K] x [n, K]ᵀ -> [M, n_pad],
// n = 2 r = 16 .. 128, K = 4096.  A skinny-N problem none of the tiled GEMMs serves (they need N % 128 == 0 and walk the whole K per
// tile: a handful of workgroups at M = 576).  Here one workgroup owns 32 rows x ALL n_pad columns x ONE slice of K:
//
//   grid (ceil(M / 32), ks), 4 waves per workgroup, every wave a quarter of the workgroup's K slice; operands go from global memory straight
//   into MFMA fragments (each lane reads 64 contiguous bytes of its row per 128-byte panel: whole cache lines, no LDS staging — every byte of
//   x is used exactly once, A [n, K] is <= 1 MiB and stays in L2);
//   the 4 waves' accumulators are summed through LDS in the fixed order ((w0 + w1) + w2) + w3;
//   ks > 1: the fp32 partial of K slice z goes to workspace[z][M][n_pad] and a second launch adds the slices in the order z = 0, 1, ... —
//   no float atomics anywhere: the result is a function of (M, K, n_pad, dtype) and the inputs only, bit for bit.
//
// Columns [n, n_pad) of the output are written as zeros (the fragment of a row of A beyond n is zero): the caller's buffer is the K
// extension of the QKV GEMM's A operand (stllm_llama_layers_lora), whose pad columns meet zero weights and must not hold NaN bit patterns.
#include "common.h"

#include <type_traits>

namespace {

constexpr int kRows = 32;      // rows of x per workgroup (one 32x32 MFMA tile in M)
constexpr int kWaves = 4;
constexpr int kPanel = 128;    // bytes of K per row and step: 64 per lane half = 4 MFMA fragments of 16 bytes

// K slices: enough workgroups for the 256 CUs, at least 2 panels per wave
inline int lora_down_ks(int M, int panels) {
  const int tiles = (M + kRows - 1) / kRows;
  int ks = 1;
  while (ks < 32 && tiles * ks < 256 && panels / (2 * ks) >= 2 * kWaves) ks *= 2;
  return ks;
}

template <typename T, int NB>
__global__ __launch_bounds__(64 * kWaves) void lora_down_kernel(const char* x, int64_t ldx_b, const char* A, int64_t lda_b, void* out, int64_t ldo,
                                                                float* part, int M, int n, int panels, int ks) {
  __shared__ float red[kWaves - 1][kRows][NB * 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * kRows, kz = blockIdx.y;
  const int units = ks * kWaves, u = kz * kWaves + wave;
  const int p0 = (int)((int64_t)panels * u / units), p1 = (int)((int64_t)panels * (u + 1) / units);
  int row = m0 + li;
  if (row >= M) row = M - 1;   // rows past the end read the last row; their results are never stored
  const char* xp = x + (int64_t)row * ldx_b + lh * 64;
  const char* ap[NB];
  bool live[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int c = j * 32 + li;
    live[j] = c < n;
    ap[j] = A + (int64_t)(live[j] ? c : 0) * lda_b + lh * 64;
  }
  f32x16 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
  const i32x4 zero = {0, 0, 0, 0};
  for (int p = p0; p < p1; ++p) {
    const int64_t off = (int64_t)p * kPanel;
    i32x4 xf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) xf[s] = *reinterpret_cast<const i32x4*>(xp + off + s * 16);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      i32x4 wf[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) wf[s] = live[j] ? *reinterpret_cast<const i32x4*>(ap[j] + off + s * 16) : zero;
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[j] = Elem<T>::mfma(xf[s], wf[s], acc[j]);   // the k <-> fragment slot map is the same for both operands
    }
  }
  // C layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wave - 1][(r & 3) + 8 * (r >> 2) + 4 * lh][j * 32 + li] = acc[j][r];
  }
  __syncthreads();
  if (wave == 0) {
    constexpr int NP = NB * 32;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ri = (r & 3) + 8 * (r >> 2) + 4 * lh, c = j * 32 + li, m = m0 + ri;
        float v = acc[j][r];
#pragma unroll
        for (int w = 0; w < kWaves - 1; ++w) v += red[w][ri][c];
        if (m < M) {
          if (ks == 1) store_elem<T>(out, (int64_t)m * ldo + c, v);
          else part[((int64_t)kz * M + m) * NP + c] = v;
        }
      }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void lora_down_reduce_kernel(const float* part, void* out, int64_t ldo, int M, int np, int ks) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)M * np;
  if (i >= total) return;
  float v = part[i];
  for (int z = 1; z < ks; ++z) v += part[(int64_t)z * total + i];
  store_elem<T>(out, (i / np) * ldo + (i % np), v);
}

template <typename T, int NB>
int launch_down(const char* x, int64_t ldx_b, const char* A, int64_t lda_b, void* out, int64_t ldo, float* part, int M, int n, int panels, int ks,
                hipStream_t stream) {
  hipLaunchKernelGGL((lora_down_kernel<T, NB>), dim3((M + kRows - 1) / kRows, ks), dim3(64 * kWaves), 0, stream, x, ldx_b, A, lda_b, out, ldo, part, M, n,
                     panels, ks);
  STLLM_CHECK_LAUNCH("stllm_lora_down");
  if (ks > 1) {
    const int64_t total = (int64_t)M * NB * 32;
    hipLaunchKernelGGL(lora_down_reduce_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, out, ldo, M, NB * 32, ks);
    STLLM_CHECK_LAUNCH("stllm_lora_down(reduce)");
  }
  return STLLM_OK;
}

template <typename T>
int dispatch_down(int nb, const char* x, int64_t ldx_b, const char* A, int64_t lda_b, void* out, int64_t ldo, float* part, int M, int n, int panels, int ks,
                  hipStream_t stream) {
  switch (nb) {
    case 1: return launch_down<T, 1>(x, ldx_b, A, lda_b, out, ldo, part, M, n, panels, ks, stream);
    case 2: return launch_down<T, 2>(x, ldx_b, A, lda_b, out, ldo, part, M, n, panels, ks, stream);
    case 3: return launch_down<T, 3>(x, ldx_b, A, lda_b, out, ldo, part, M, n, panels, ks, stream);
    default: return launch_down<T, 4>(x, ldx_b, A, lda_b, out, ldo, part, M, n, panels, ks, stream);
  }
}

inline int down_esize(int dtype) { return dtype == STLLM_F32 ? 4 : 2; }

}  // namespace

extern "C" int64_t stllm_lora_down_workspace_bytes(int dtype, int M, int K, int n_pad) {
  if ((dtype != STLLM_BF16 && dtype != STLLM_F16 && dtype != STLLM_F32) || M <= 0 || K <= 0 || n_pad <= 0 || n_pad % 32 != 0 || n_pad > 128 ||
      ((int64_t)K * down_esize(dtype)) % kPanel != 0)
    return -1;
  const int ks = lora_down_ks(M, (int)((int64_t)K * down_esize(dtype) / kPanel));
  return ks == 1 ? 0 : (int64_t)ks * M * n_pad * 4;
}

extern "C" int stllm_lora_down(int dtype, const void* x, int64_t ldx, const void* A, int64_t lda, void* out, int64_t ldo, int M, int K, int n, int n_pad,
                               void* workspace, int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (dtype != STLLM_BF16 && dtype != STLLM_F16 && dtype != STLLM_F32) {
    stllm_set_error("stllm_lora_down: dtype %d (bf16 / fp16 / fp32 only: merge the adapters for the split modes)", dtype);
    return STLLM_ERR_BAD_DTYPE;
  }
  const int eb = down_esize(dtype);
  STLLM_CHECK_ARG(x && A && out && M > 0 && K > 0, "stllm_lora_down: null / empty arguments (M=%d K=%d)", M, K);
  STLLM_CHECK_ARG(n >= 1 && n <= n_pad && n_pad % 32 == 0 && n_pad <= 128, "stllm_lora_down: need 1 <= n <= n_pad <= 128, n_pad %% 32 == 0 (n=%d n_pad=%d)", n, n_pad);
  STLLM_CHECK_ARG(((int64_t)K * eb) % kPanel == 0, "stllm_lora_down: K=%d must be a whole number of 128-byte panels", K);
  STLLM_CHECK_ARG(aligned16(x) && aligned16(A) && (ldx * eb) % 16 == 0 && (lda * eb) % 16 == 0 && ldx >= K && lda >= K && ldo >= n_pad,
                  "stllm_lora_down: misaligned operands or short rows (ldx=%lld lda=%lld ldo=%lld)", (long long)ldx, (long long)lda, (long long)ldo);
  {   // out may share ROWS with x (the K-extended operand: out = x + K, same row stride) but never bytes: any other overlap would race
    const char* xb = reinterpret_cast<const char*>(x);
    const char* ob = reinterpret_cast<const char*>(out);
    const int64_t span_x = ((int64_t)(M - 1) * ldx + K) * eb, span_o = ((int64_t)(M - 1) * ldo + n_pad) * eb, d = ob - xb;
    if (ob < xb + span_x && xb < ob + span_o)
      STLLM_CHECK_ARG(ldx == ldo && d >= (int64_t)K * eb && d + (int64_t)n_pad * eb <= ldx * eb,
                      "stllm_lora_down: out overlaps x (allowed only as columns behind K of the same rows: ldx == ldo, K <= offset, offset + n_pad <= ldx)");
    STLLM_CHECK_ARG((reinterpret_cast<uintptr_t>(out) % eb) == 0, "stllm_lora_down: misaligned out");
  }
  const int panels = (int)((int64_t)K * eb / kPanel), ks = lora_down_ks(M, panels);
  const int64_t need = ks == 1 ? 0 : (int64_t)ks * M * n_pad * 4;
  STLLM_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0),
                  "stllm_lora_down: workspace of %lld bytes needed, %lld given", (long long)need, (long long)workspace_bytes);
  const char* xc = reinterpret_cast<const char*>(x);
  const char* ac = reinterpret_cast<const char*>(A);
  float* part = reinterpret_cast<float*>(workspace);
  int rc;
  switch (dtype) {
    case STLLM_BF16: rc = dispatch_down<bf16_t>(n_pad / 32, xc, ldx * eb, ac, lda * eb, out, ldo, part, M, n, panels, ks, stream); break;
    case STLLM_F16: rc = dispatch_down<f16_t>(n_pad / 32, xc, ldx * eb, ac, lda * eb, out, ldo, part, M, n, panels, ks, stream); break;
    default: rc = dispatch_down<float>(n_pad / 32, xc, ldx * eb, ac, lda * eb, out, ldo, part, M, n, panels, ks, stream); break;
  }
  if (rc == STLLM_OK) stllm_set_last_kernel(dtype == STLLM_BF16 ? "lora_down_kernel<bf16_t>" : dtype == STLLM_F16 ? "lora_down_kernel<f16_t>" : "lora_down_kernel<float>");
  return rc;
}
