// Feature-space (F/W+) inversion of the StyleGAN2 generator: the layout kernels between the
// NCHW tensors of the Python surface and the NHWC activations of the synthesis workspace, and the regulariser that
// keeps an optimised activation near its start.
//
// Transposes.  [Bn][C][H][W] <-> [Bn][H][W][C] is, per image, the transpose of a (rows x cols) matrix: rows = H W,
// cols = C one way, rows = C, cols = H W the other.  One block moves a 64 x 64 tile through LDS (pitch 65: the
// column reads of the store phase hit 64 different banks): 64 consecutive floats of a source row are read by
// consecutive lanes and 64 consecutive floats of a destination row are written by consecutive lanes, so both sides
// are coalesced.  Each side uses 16-byte accesses when its row length is a multiple of 4 and its pointer is 16-byte
// aligned (every row then starts on a 16-byte boundary, and a float4 lies wholly inside or wholly outside the
// matrix); otherwise that side uses 4-byte accesses.  The tile edge is guarded on both sides.  No workspace.
//
// FeatureAnchor.  f [Bn][n] fp32, anchor a [n] (stride 0: shared) or [Bn][n]:
//   loss[b] = weight (1 / n) sum_i (f[b,i] - a[i])^2,   df[b,i] = gloss[b] (2 weight / n) (f[b,i] - a[i])
// f - a is exact in fp64 (two fp32 values), squares and sums are fp64 (v_fma_f64), loss and df are rounded once.
//   forward, 2 launches:  partial  block (chunk, b) takes the 4096 elements from 4096 chunk: thread t walks
//                                  t, t + 256, ... (16 steps, loads in flight together, one fma chain in step order;
//                                  an element past n adds fma(0, 0, s) = s), a butterfly adds the 64 lanes, the 4 waves
//                                  are added in order; the partial goes to the workspace ([b][chunk], fp64).
//                         finish   one block per candidate: thread t adds the partials t, t + 256, ... in order,
//                                  butterfly, waves in order, weight * (sum / n), rounded to fp32.
//   backward, 1 launch:   elementwise; gloss[b] is the LAST factor, so gloss = 2 or -1 scale the result bit for bit.
// The order of every sum follows from n alone: a candidate's loss and gradient do not depend on Bn, on its row, on the
// stream or on the call.  No atomics, no memset.
#include <limits.h>
#include "p2l_common.h"

namespace {

constexpr int kTile = 64;
constexpr int kThreads = 256;
constexpr int kChunk = 4096;                    // elements of a candidate per block of the partial launch
constexpr int kSteps = kChunk / kThreads;       // 16

bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }
bool aligned8(const void* a) { return ((uintptr_t)a & 7) == 0; }

// dst[b][c][r] = src[b][r][c], r < R, c < Cn.  VL: 16-byte loads (Cn % 4 == 0), VS: 16-byte stores (R % 4 == 0)
template <bool VL, bool VS>
__global__ __launch_bounds__(kThreads) void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                             int R, int Cn) {
  __shared__ float tile[kTile][kTile + 1];
  const size_t base = (size_t)blockIdx.z * (size_t)R * (size_t)Cn;
  const float* s = src + base;
  float* d = dst + base;
  const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile, tid = threadIdx.x;
  if (VL) {
    const int cq = tid & 15, rr = tid >> 4;            // 16 float4 per tile row, 16 rows per pass
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int tr = rr + 16 * p, r = r0 + tr, c = c0 + 4 * cq;
      if (r < R && c < Cn) {                           // (Cn % 4 == 0: c < Cn means c + 3 < Cn)
        const float4 v = *(const float4*)(s + (size_t)r * Cn + c);
        tile[tr][4 * cq + 0] = v.x; tile[tr][4 * cq + 1] = v.y;
        tile[tr][4 * cq + 2] = v.z; tile[tr][4 * cq + 3] = v.w;
      }
    }
  } else {
    const int cc = tid & 63, rr = tid >> 6;            // a wave reads 64 consecutive floats of one row
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int tr = rr + 4 * p, r = r0 + tr, c = c0 + cc;
      if (r < R && c < Cn) tile[tr][cc] = s[(size_t)r * Cn + c];
    }
  }
  __syncthreads();
  if (VS) {
    const int rq = tid & 15, cc = tid >> 4;            // 16 float4 per destination row of the tile
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int tc = cc + 16 * p, c = c0 + tc, r = r0 + 4 * rq;
      if (c < Cn && r < R) {                           // (R % 4 == 0: r < R means r + 3 < R)
        float4 v;
        v.x = tile[4 * rq + 0][tc]; v.y = tile[4 * rq + 1][tc];
        v.z = tile[4 * rq + 2][tc]; v.w = tile[4 * rq + 3][tc];
        *(float4*)(d + (size_t)c * R + r) = v;
      }
    }
  } else {
    const int rr = tid & 63, cc = tid >> 6;            // a wave writes 64 consecutive floats of one row
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int tc = cc + 4 * p, c = c0 + tc, r = r0 + rr;
      if (c < Cn && r < R) d[(size_t)c * R + r] = tile[rr][tc];
    }
  }
}

int transpose_launch(const float* src, float* dst, int Bn, int64_t R64, int64_t C64, void* stream) {
  if (!src || !dst || Bn < 1 || R64 < 1 || C64 < 1 || R64 > INT_MAX || C64 > INT_MAX) return P2L_EINVAL;
  const int R = (int)R64, Cn = (int)C64;
  const int gx = cdiv(Cn, kTile), gy = cdiv(R, kTile);
  if (Bn > 65535 || gy > 65535) return P2L_EINVAL;      // (grid y / z: H W <= 4 M, or C <= 4 M)
  const bool vl = (Cn % 4 == 0) && aligned16(src), vs = (R % 4 == 0) && aligned16(dst);
  const dim3 grid(gx, gy, Bn), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (vl && vs) hipLaunchKernelGGL((transpose_kernel<true, true>), grid, block, 0, st, src, dst, R, Cn);
  else if (vl) hipLaunchKernelGGL((transpose_kernel<true, false>), grid, block, 0, st, src, dst, R, Cn);
  else if (vs) hipLaunchKernelGGL((transpose_kernel<false, true>), grid, block, 0, st, src, dst, R, Cn);
  else hipLaunchKernelGGL((transpose_kernel<false, false>), grid, block, 0, st, src, dst, R, Cn);
  return p2l_check_launch();
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

__global__ __launch_bounds__(kThreads) void fa_partial_kernel(const float* __restrict__ f,
                                                              const float* __restrict__ anchor, long long a_bstride,
                                                              long long n, int nchunk, double* __restrict__ part) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const float* fb = f + (size_t)b * n;
  const float* ab = anchor + (size_t)b * a_bstride;
  const long long i0 = (long long)chunk * kChunk + tid;
  float x[kSteps], a[kSteps];
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const long long i = i0 + (long long)k * kThreads;
    x[k] = i < n ? fb[i] : 0.0f;
    a[k] = i < n ? ab[i] : 0.0f;
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const double d = (double)x[k] - (double)a[k];
    s = fma(d, d, s);
  }
  s = block_sum_f64(s, red);
  if (tid == 0) part[(size_t)b * nchunk + chunk] = s;
}

__global__ __launch_bounds__(kThreads) void fa_finish_kernel(const double* __restrict__ part, int nchunk, long long n,
                                                             double weight, float* __restrict__ loss) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* pb = part + (size_t)b * nchunk;
  double s = 0.0;
  for (int c = tid; c < nchunk; c += kThreads) s += pb[c];
  s = block_sum_f64(s, red);
  if (tid == 0) loss[b] = (float)(weight * (s / (double)n));
}

__global__ __launch_bounds__(kThreads) void fa_bwd_kernel(const float* __restrict__ f, const float* __restrict__ anchor,
                                                          long long a_bstride, const float* __restrict__ gloss,
                                                          long long n, double weight, float* __restrict__ df) {
  const int b = blockIdx.y;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double gl = gloss ? (double)gloss[b] : 1.0;
  const double scale = (2.0 * weight) / (double)n;
  const double d = (double)f[(size_t)b * n + i] - (double)anchor[(size_t)b * a_bstride + i];
  df[(size_t)b * n + i] = (float)((scale * d) * gl);
}

bool fa_shape_ok(int Bn, int64_t n, int64_t a_bstride) {
  // (grid x of the partial launch = n / 4096, of the backward n / 256: far inside an int for n < 2^31)
  return Bn >= 1 && Bn <= 65535 && n >= 1 && n <= INT_MAX && (a_bstride == 0 || a_bstride >= n);
}
size_t fa_ws_bytes(int Bn, int64_t n) { return (size_t)Bn * (size_t)cdiv(n, kChunk) * sizeof(double); }

}  // namespace

extern "C" int p2l_nhwc_to_nchw(const float* src, float* dst, int Bn, int C, int H, int W, void* stream) {
  if (C < 1 || H < 1 || W < 1) return P2L_EINVAL;
  return transpose_launch(src, dst, Bn, (int64_t)H * W, C, stream);
}

extern "C" int p2l_nchw_to_nhwc(const float* src, float* dst, int Bn, int C, int H, int W, void* stream) {
  if (C < 1 || H < 1 || W < 1) return P2L_EINVAL;
  return transpose_launch(src, dst, Bn, C, (int64_t)H * W, stream);
}

extern "C" size_t p2l_feature_anchor_ws_bytes(int Bn, int64_t n) {
  if (!fa_shape_ok(Bn, n, 0)) return 0;
  return fa_ws_bytes(Bn, n);
}

extern "C" int p2l_feature_anchor_fwd(const float* f, const float* anchor, int64_t anchor_bstride, int Bn, int64_t n,
                                      double weight, float* loss, void* ws, size_t ws_bytes, void* stream) {
  if (!f || !anchor || !loss || !fa_shape_ok(Bn, n, anchor_bstride)) return P2L_EINVAL;
  if (!ws || !aligned8(ws) || ws_bytes < fa_ws_bytes(Bn, n)) return P2L_EWS;
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = cdiv(n, kChunk);
  double* part = (double*)ws;
  hipLaunchKernelGGL(fa_partial_kernel, dim3(nchunk, Bn), dim3(kThreads), 0, st, f, anchor, (long long)anchor_bstride,
                     (long long)n, nchunk, part);
  hipLaunchKernelGGL(fa_finish_kernel, dim3(Bn), dim3(kThreads), 0, st, part, nchunk, (long long)n, weight, loss);
  return p2l_check_launch();
}

extern "C" int p2l_feature_anchor_bwd(const float* f, const float* anchor, int64_t anchor_bstride, const float* gloss,
                                      int Bn, int64_t n, double weight, float* df, void* stream) {
  if (!f || !anchor || !df || !fa_shape_ok(Bn, n, anchor_bstride)) return P2L_EINVAL;
  hipLaunchKernelGGL(fa_bwd_kernel, dim3(cdiv(n, kThreads), Bn), dim3(kThreads), 0, (hipStream_t)stream, f, anchor,
                     (long long)anchor_bstride, gloss, (long long)n, weight, df);
  return p2l_check_launch();
}
