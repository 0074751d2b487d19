// StyleSpace (S) search of the StyleGAN2 generator: the way into and out of the style slots of
// the synthesis workspace, the channel statistics, and the diagonal prior that keeps the free variable where the
// generator was trained.
//
// Layout.  A candidate's styles are one flat vector [S_total] in network order: conv[0], rgb[0], then per resolution
// the up conv, the plain conv and their ToRGB; a layer's entry is its cin modulation scalars (p2l_sg2_style_layout).
//
// Scatter / gather.  One launch each, whatever Bn and the layer count are: block (tile, layer, candidate) copies up
// to 256 consecutive floats between the candidate's slice of the flat vector and the layer's [Bn][cin] slot of the
// workspace.  Every element has one writer: no atomics.
//
// Column moments.  x [rows][ld] -> sum[c], sumsq[c] in fp64.  One thread owns a column and adds its rows in row order
// (x -> fp64 and x * x are exact: 24-bit significands), 16 loads in flight; with accumulate the two chains start from
// what the outputs hold, so a sample set streamed in chunks gives the bits of one call over all its rows.
//
// Diagonal prior.  loss[b] = weight (1 / n) sum_i ((x[b,i] - c[i]) r[i])^2, the two-launch shape of the FeatureAnchor
// term (csrc/p2l_sg2_feat.hip): 4096-element chunks, thread t walks t, t + 256, ... with one fma chain, butterfly over
// the 64 lanes, the 4 waves in order, partials [b][chunk] in the workspace; the finish adds them in order.  The backward
// is elementwise with gloss[b] as the LAST factor.
#include <limits.h>
#include "p2l_common.h"
#include "p2l_sg2_k.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;
constexpr int kSteps = kChunk / kThreads;       // 16
constexpr int kColThreads = 64;
constexpr int kRowsInFlight = 16;

bool aligned8(const void* a) { return ((uintptr_t)a & 7) == 0; }

// to_ws = 1: ws slot <- flat (scatter of the styles); 0: flat <- ws slot (gather of their gradients)
template <int TO_WS>
__global__ __launch_bounds__(kThreads) void style_move_kernel(const p2lsg2::StyleMoveK k) {
  const p2lsg2::StyleMoveItem g = k.g[blockIdx.y];
  const int c = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.z;
  if (c >= g.cin) return;
  float* slot = g.slot + (size_t)b * g.cin + c;
  float* flat = k.flat + (size_t)b * k.total + g.off + c;
  if (TO_WS) *slot = *flat; else *flat = *slot;
}

__global__ __launch_bounds__(kColThreads) void col_moments_kernel(const float* __restrict__ x, long long rows, int cols,
                                                                  long long ld, double* __restrict__ sum,
                                                                  double* __restrict__ sumsq, int accumulate) {
  const int c = blockIdx.x * kColThreads + threadIdx.x;
  if (c >= cols) return;
  double s = accumulate ? sum[c] : 0.0, q = accumulate ? sumsq[c] : 0.0;
  const float* p = x + c;
  long long r = 0;
  for (; r + kRowsInFlight <= rows; r += kRowsInFlight) {
    float v[kRowsInFlight];
#pragma unroll
    for (int i = 0; i < kRowsInFlight; ++i) v[i] = p[(size_t)(r + i) * ld];
#pragma unroll
    for (int i = 0; i < kRowsInFlight; ++i) {
      const double d = (double)v[i];
      s += d;
      q += d * d;                  // (the product is exact; mul then add: the same two roundings as numpy's)
    }
  }
  for (; r < rows; ++r) {
    const double d = (double)p[(size_t)r * ld];
    s += d;
    q += d * d;
  }
  sum[c] = s;
  sumsq[c] = q;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the 256 values of a block: butterfly per wave, then the 4 waves in order (valid in thread 0)
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum_f64(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kThreads) void dp_partial_kernel(const float* __restrict__ x,
                                                              const double* __restrict__ center,
                                                              const double* __restrict__ inv_scale, long long n,
                                                              int nchunk, double* __restrict__ part) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const float* xb = x + (size_t)b * n;
  const long long i0 = (long long)chunk * kChunk + tid;
  float v[kSteps];
  double c[kSteps], r[kSteps];
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const long long i = i0 + (long long)k * kThreads;
    v[k] = i < n ? xb[i] : 0.0f;
    c[k] = i < n ? center[i] : 0.0;
    r[k] = i < n ? inv_scale[i] : 0.0;         // (an element past n adds fma(0, 0, s) = s)
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const double d = ((double)v[k] - c[k]) * r[k];
    s = fma(d, d, s);
  }
  s = block_sum_f64(s, red);
  if (tid == 0) part[(size_t)b * nchunk + chunk] = s;
}

__global__ __launch_bounds__(kThreads) void dp_finish_kernel(const double* __restrict__ part, int nchunk, long long n,
                                                             double weight, float* __restrict__ loss) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* pb = part + (size_t)b * nchunk;
  double s = 0.0;
  for (int c = tid; c < nchunk; c += kThreads) s += pb[c];
  s = block_sum_f64(s, red);
  if (tid == 0) loss[b] = (float)(weight * (s / (double)n));
}

__global__ __launch_bounds__(kThreads) void dp_bwd_kernel(const float* __restrict__ x, const double* __restrict__ center,
                                                          const double* __restrict__ inv_scale,
                                                          const float* __restrict__ gloss, long long n, double weight,
                                                          float* __restrict__ dx) {
  const int b = blockIdx.y;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double gl = gloss ? (double)gloss[b] : 1.0;
  const double scale = (2.0 * weight) / (double)n;
  const double r = inv_scale[i];
  const double d = ((double)x[(size_t)b * n + i] - center[i]) * r;
  dx[(size_t)b * n + i] = (float)(((scale * d) * r) * gl);
}

bool dp_shape_ok(int Bn, int64_t n) { return Bn >= 1 && Bn <= 65535 && n >= 1 && n <= INT_MAX; }
size_t dp_ws_bytes(int Bn, int64_t n) { return (size_t)Bn * (size_t)cdiv(n, kChunk) * sizeof(double); }

}  // namespace

namespace p2lsg2 {

int style_move(const StyleMoveK& k, int to_ws, void* stream) {
  if (k.n < 1 || k.n > STYLE_MAX || k.Bn < 1 || k.Bn > 65535 || !k.flat || k.total < 1) return P2L_EINVAL;
  int maxc = 0;
  for (int i = 0; i < k.n; ++i) {
    const StyleMoveItem& g = k.g[i];
    if (!g.slot || g.cin < 1 || g.off < 0 || g.off + g.cin > k.total) return P2L_EINVAL;
    if (g.cin > maxc) maxc = g.cin;
  }
  const dim3 grid(cdiv(maxc, kThreads), k.n, k.Bn), block(kThreads);
  if (to_ws) hipLaunchKernelGGL(style_move_kernel<1>, grid, block, 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL(style_move_kernel<0>, grid, block, 0, (hipStream_t)stream, k);
  return p2l_check_launch();
}

}  // namespace p2lsg2

extern "C" int p2l_sg2_style_layout(const P2LStyleGAN2* m, int32_t* conv_off, int32_t* rgb_off, int32_t* total) {
  if (!m || m->n_conv < 1 || m->n_conv > P2L_SG2_MAX_CONVS || m->n_rgb < 0 || m->n_rgb > P2L_SG2_MAX_RGBS)
    return P2L_EINVAL;
  int64_t off = 0;
  int rj = 0;
  for (int l = 0; l < m->n_conv; ++l) {
    if (m->conv[l].cin < 1) return P2L_EINVAL;
    if (conv_off) conv_off[l] = (int32_t)off;
    off += m->conv[l].cin;
    while (rj < m->n_rgb && m->rgb[rj].after_conv == l) {
      if (m->rgb[rj].cin < 1) return P2L_EINVAL;
      if (rgb_off) rgb_off[rj] = (int32_t)off;
      off += m->rgb[rj].cin;
      ++rj;
    }
    if (off > INT_MAX) return P2L_EINVAL;
  }
  if (rj != m->n_rgb) return P2L_EINVAL;          // a ToRGB that follows no conv (or out of order)
  if (total) *total = (int32_t)off;
  return P2L_OK;
}

extern "C" int p2l_col_moments_f64(const float* x, int64_t rows, int cols, int64_t ld, double* sum, double* sumsq,
                                   int accumulate, void* stream) {
  if (!x || !sum || !sumsq || rows < 1 || cols < 1 || ld < cols) return P2L_EINVAL;
  if (rows > ((int64_t)1 << 62) / ld) return P2L_EINVAL;
  hipLaunchKernelGGL(col_moments_kernel, dim3(cdiv(cols, kColThreads)), dim3(kColThreads), 0, (hipStream_t)stream, x,
                     (long long)rows, cols, (long long)ld, sum, sumsq, accumulate ? 1 : 0);
  return p2l_check_launch();
}

extern "C" size_t p2l_diag_prior_ws_bytes(int Bn, int64_t n) {
  if (!dp_shape_ok(Bn, n)) return 0;
  return dp_ws_bytes(Bn, n);
}

extern "C" int p2l_diag_prior_fwd(const float* x, const double* center, const double* inv_scale, int Bn, int64_t n,
                                  double weight, float* loss, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !center || !inv_scale || !loss || !dp_shape_ok(Bn, n)) return P2L_EINVAL;
  if (!ws || !aligned8(ws) || ws_bytes < dp_ws_bytes(Bn, n)) return P2L_EWS;
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = cdiv(n, kChunk);
  double* part = (double*)ws;
  hipLaunchKernelGGL(dp_partial_kernel, dim3(nchunk, Bn), dim3(kThreads), 0, st, x, center, inv_scale, (long long)n,
                     nchunk, part);
  hipLaunchKernelGGL(dp_finish_kernel, dim3(Bn), dim3(kThreads), 0, st, part, nchunk, (long long)n, weight, loss);
  return p2l_check_launch();
}

extern "C" int p2l_diag_prior_bwd(const float* x, const double* center, const double* inv_scale, const float* gloss,
                                  int Bn, int64_t n, double weight, float* dx, void* stream) {
  if (!x || !center || !inv_scale || !dx || !dp_shape_ok(Bn, n)) return P2L_EINVAL;
  hipLaunchKernelGGL(dp_bwd_kernel, dim3(cdiv(n, kThreads), Bn), dim3(kThreads), 0, (hipStream_t)stream, x, center,
                     inv_scale, gloss, (long long)n, weight, dx);
  return p2l_check_launch();
}
