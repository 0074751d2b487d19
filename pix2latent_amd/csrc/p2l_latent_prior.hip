// Whitened-PCA prior on a latent (the P_N / P_N+ term of "Improved StyleGAN Embedding",
// Zhu et al. 2020, generalised to any basis / mean / layer weights).
//
// w [B][L][D] fp32, basis A [K][D] fp64, mean m [D] fp64, layer weights a [L] fp64, flag p_space:
//   x = (p_space && w < 0) ? 5 w : w          (fp64, exact; -0.0 and 0 take slope 1)
//   d = x - m,   v[b,l,k] = sum_j A[k,j] d[b,l,j],   P[b] = sum_l a_l (1 / K) sum_k v[b,l,k]^2
//   dw[b,l,j] = gloss[b] slope(w[b,l,j]) (2 a_l / K) sum_k A[k,j] v[b,l,k]
// Everything is fp64 (v_fma_f64); P and dw are rounded once to fp32.
//
// Launches (blockIdx.y is the candidate; no atomics, no memset, nothing waits for the host):
//   forward, 2:   project  one block per (8 rows of a candidate, 64 components).  The 8 rows of d go to LDS as fp64
//                          ([j][row], 32 KB at D = 512: a lane reads the 8 rows of one j as four 16-byte broadcasts);
//                          lane = component, wave q walks the q-th quarter of j in order with 8 accumulators (one per
//                          row) and reads A TRANSPOSED ([D][K]: the 64 lanes of a wave read 64 consecutive doubles);
//                          the four quarters are added ((q0 + q1) + q2) + q3 and v goes to the workspace.
//                 finish   one block of 16 waves per candidate: wave q takes the layers l = q, q + 16, ...; a lane
//                          sums v[k]^2 over k = lane, lane + 64, ..., a butterfly adds the lanes, the wave adds
//                          a_l (s / K) in layer order, and the 16 waves are added in order.
//   backward, 1:  the mirror image of `project`: 8 rows of v in LDS ([k][row]), lane = column j, wave q walks the
//                 q-th quarter of k (quarters of ceil(K / 4)) and reads A as it is ([K][D]); the epilogue applies
//                 slope, 2 a_l / K and LAST gloss[b] (so that gloss = 2 or -1 scale the result bit for bit).
// The order of every sum is a function of (D, K, L) alone: a candidate's P and dw do not depend on B, on its row,
// on the stream or on the call.
//
// 22 x 18 rows x 512 x 512 is 0.1 G fp64 FMA each way (under 3 us at the vector fp64 rate) over 2 MB of basis that
// stays in L2: the kernels are bound by latency -- a lane's walk is D / 4 = 128 dependent steps of 8 FMAs, each
// behind an LDS read, in a grid that fills the chip about twice -- not by bandwidth (measured).
#include "p2l_common.h"

namespace {

constexpr int kThreads = 256;            // 4 waves
constexpr int kFinishThreads = 1024;     // 16 waves: one block per candidate, a wave per layer (mod 16)
constexpr int kRows = 8;                 // rows of a candidate per block
constexpr int kCols = 64;                // components (forward) / columns (backward) per block: one per lane
constexpr int kMaxD = 512;
constexpr int kBatch = 16;               // steps of a walk whose loads of the basis are issued together
constexpr int kMaxL = 1 << 20;           // keeps the 1-D grid of (row chunk, column block) far inside an int

bool lp_shape_ok(int B, int L, int D, int K) {
  return B >= 1 && B <= 65535 && L >= 1 && L <= kMaxL && K >= 1 && D >= kCols && D <= kMaxD && D % kCols == 0 &&
         K <= D;
}
size_t lp_ws_bytes(int B, int L, int K) { return (size_t)B * L * K * sizeof(double); }
bool aligned8(const void* a) { return ((uintptr_t)a & 7) == 0; }
bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// acc[r] += sum over the steps [s0, s1) of M[s * ld + col] * rows[s][r]: one chain per row, in step order
__device__ __forceinline__ void lp_walk(const double* __restrict__ M, int ld, int col, int s0, int s1,
                                        const double (*rows)[kRows], double (&acc)[kRows]) {
  const double* mp = M + (size_t)s0 * ld + col;
  int s = s0;
  // kBatch loads of M in flight together, then their FMAs: the chains keep the step order
  for (; s + kBatch <= s1; s += kBatch, mp += (size_t)kBatch * ld) {
    double a[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) a[i] = mp[(size_t)i * ld];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) acc[r] = fma(a[i], rows[s + i][r], acc[r]);
    }
  }
  for (; s < s1; ++s, mp += ld) {
    const double a = *mp;
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = fma(a, rows[s][r], acc[r]);
  }
}

// v[b, l0 .. l0 + 7, kb * 64 .. + 63]
__global__ __launch_bounds__(kThreads) void lp_project_kernel(const float* __restrict__ w,
                                                              const double* __restrict__ basis_t,
                                                              const double* __restrict__ mean, int L, int D, int K,
                                                              int p_space, int nkb, double* __restrict__ v) {
  __shared__ __attribute__((aligned(16))) double sd[kMaxD][kRows];
  __shared__ double part[4][kRows][kCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = blockIdx.x / nkb, kb = blockIdx.x - lc * nkb, b = blockIdx.y;
  const int l0 = lc * kRows;
  const int nrows = L - l0 < kRows ? L - l0 : kRows;
  const size_t row0 = (size_t)b * L + l0;

  // 8 rows x D / 4 float4: lane = (row, float4) with the row fastest (the LDS image is [j][row]).  A row past the
  // candidate's last re-reads that last row and stores zeros: every load is unconditional and the loop's loads
  // are in flight together
  const int nq = D >> 2;
#pragma unroll 4
  for (int idx = tid; idx < kRows * nq; idx += kThreads) {
    const int r = idx & (kRows - 1), q = idx >> 3;
    const int rr = r < nrows ? r : nrows - 1;
    const float4 x4 = *(const float4*)(w + (row0 + rr) * D + 4 * q);
    const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double xd = (double)xs[i];
      if (p_space && xs[i] < 0.0f) xd *= 5.0;
      const double d = xd - mean[4 * q + i];
      sd[4 * q + i][r] = r < nrows ? d : 0.0;
    }
  }
  __syncthreads();

  double acc[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) acc[r] = 0.0;
  // (a lane past K walks column K - 1 and stores nothing: no divergent region around the loop, whose loads the
  // compiler then keeps in flight together)
  const int k = kb * kCols + lane < K ? kb * kCols + lane : K - 1;
  const int jq = D >> 2;
  lp_walk(basis_t, K, k, wave * jq, (wave + 1) * jq, sd, acc);
#pragma unroll
  for (int r = 0; r < kRows; ++r) part[wave][r][lane] = acc[r];
  __syncthreads();

  for (int idx = tid; idx < kRows * kCols; idx += kThreads) {
    const int r = idx >> 6, c = idx & 63, kk = kb * kCols + c;
    if (r < nrows && kk < K)
      v[(row0 + r) * K + kk] = ((part[0][r][c] + part[1][r][c]) + part[2][r][c]) + part[3][r][c];
  }
}

__global__ __launch_bounds__(kFinishThreads) void lp_finish_kernel(const double* __restrict__ v,
                                                                   const double* __restrict__ layer_w, int L, int K,
                                                                   float* __restrict__ loss) {
  constexpr int kWaves = kFinishThreads / 64;
  __shared__ double red[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const double inv_k = 1.0 / (double)K;
  double p = 0.0;
  for (int l = wave; l < L; l += kWaves) {
    const double* vr = v + ((size_t)b * L + l) * K;
    // K <= 512: 8 loads in flight, zeros past K (fma(0, 0, s) is s)
    double x[kMaxD / 64];
#pragma unroll
    for (int i = 0; i < kMaxD / 64; ++i) x[i] = lane + 64 * i < K ? vr[lane + 64 * i] : 0.0;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kMaxD / 64; ++i) s = fma(x[i], x[i], s);
    s = wave_sum_f64(s);
    p += layer_w[l] * (s * inv_k);
  }
  if (lane == 0) red[wave] = p;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) t += red[q];
    loss[b] = (float)t;
  }
}

// dw[b, l0 .. l0 + 7, jb * 64 .. + 63]
__global__ __launch_bounds__(kThreads) void lp_bwd_kernel(const float* __restrict__ w,
                                                          const double* __restrict__ basis,
                                                          const double* __restrict__ layer_w,
                                                          const float* __restrict__ gloss, int L, int D, int K,
                                                          int p_space, int njb, const double* __restrict__ v,
                                                          float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) double sv[kMaxD][kRows];
  __shared__ double part[4][kRows][kCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = blockIdx.x / njb, jb = blockIdx.x - lc * njb, b = blockIdx.y;
  const int l0 = lc * kRows;
  const int nrows = L - l0 < kRows ? L - l0 : kRows;
  const size_t row0 = (size_t)b * L + l0;

  // (staged as in the forward: row fastest, unconditional loads)
#pragma unroll 4
  for (int idx = tid; idx < kRows * K; idx += kThreads) {
    const int r = idx & (kRows - 1), k = idx >> 3;
    const int rr = r < nrows ? r : nrows - 1;
    const double x = v[(row0 + rr) * K + k];
    sv[k][r] = r < nrows ? x : 0.0;
  }
  __syncthreads();

  double acc[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) acc[r] = 0.0;
  const int kq = (K + 3) >> 2;
  const int k0 = wave * kq < K ? wave * kq : K;
  const int k1 = k0 + kq < K ? k0 + kq : K;
  lp_walk(basis, D, jb * kCols + lane, k0, k1, sv, acc);      // (D is a multiple of 64: every lane has a column)
#pragma unroll
  for (int r = 0; r < kRows; ++r) part[wave][r][lane] = acc[r];
  __syncthreads();

  const double gl = gloss ? (double)gloss[b] : 1.0;
  const double inv_k = 1.0 / (double)K;
  for (int idx = tid; idx < kRows * kCols; idx += kThreads) {
    const int r = idx >> 6, c = idx & 63;
    if (r < nrows) {
      const size_t o = (row0 + r) * D + jb * kCols + c;
      const double s = ((part[0][r][c] + part[1][r][c]) + part[2][r][c]) + part[3][r][c];
      const double slope = (p_space && w[o] < 0.0f) ? 5.0 : 1.0;
      const double g = slope * ((2.0 * layer_w[l0 + r]) * inv_k) * s;
      dw[o] = (float)(g * gl);
    }
  }
}

}  // namespace

extern "C" size_t p2l_latent_prior_ws_bytes(int B, int L, int K) {
  if (B < 1 || B > 65535 || L < 1 || L > kMaxL || K < 1 || K > kMaxD) return 0;
  return lp_ws_bytes(B, L, K);
}

extern "C" int p2l_latent_prior_fwd(const float* w, const double* basis_t, const double* mean, const double* layer_w,
                                    int B, int L, int D, int K, int p_space, float* loss, void* ws, size_t ws_bytes,
                                    void* stream) {
  if (!w || !aligned16(w) || !basis_t || !mean || !layer_w || !loss || !lp_shape_ok(B, L, D, K)) return P2L_EINVAL;
  if (!ws || !aligned8(ws) || ws_bytes < lp_ws_bytes(B, L, K)) return P2L_EWS;
  hipStream_t st = (hipStream_t)stream;
  const int nkb = cdiv(K, kCols), nlc = cdiv(L, kRows);
  double* v = (double*)ws;
  hipLaunchKernelGGL(lp_project_kernel, dim3(nkb * nlc, B), dim3(kThreads), 0, st, w, basis_t, mean, L, D, K,
                     p_space ? 1 : 0, nkb, v);
  hipLaunchKernelGGL(lp_finish_kernel, dim3(B), dim3(kFinishThreads), 0, st, v, layer_w, L, K, loss);
  return p2l_check_launch();
}

extern "C" int p2l_latent_prior_bwd(const float* w, const double* basis, const double* layer_w, const float* gloss,
                                    int B, int L, int D, int K, int p_space, const void* ws, size_t ws_bytes,
                                    float* dw, void* stream) {
  if (!w || !basis || !layer_w || !dw || !lp_shape_ok(B, L, D, K)) return P2L_EINVAL;
  if (!ws || !aligned8(ws) || ws_bytes < lp_ws_bytes(B, L, K)) return P2L_EWS;
  const int njb = D / kCols, nlc = cdiv(L, kRows);
  hipLaunchKernelGGL(lp_bwd_kernel, dim3(njb * nlc, B), dim3(kThreads), 0, (hipStream_t)stream, w, basis, layer_w,
                     gloss, L, D, K, p_space ? 1 : 0, njb, (const double*)ws, dw);
  return p2l_check_launch();
}
