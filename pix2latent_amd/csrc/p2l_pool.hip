// Area pooling of the image in front of the LPIPS term (`lpips_size`).
//
// pool_f(x), f in {2, 4, 8, 16}, is log2 f nested 2x2 means in fp32, each level
//   x'[y,x] = ((x[2y,2x] + x[2y,2x+1]) + (x[2y+1,2x] + x[2y+1,2x+1])) * 0.25f
// i.e. the pooled value of an f x f block is that of its four f/2 x f/2 quadrants: upper left, upper right, lower left,
// lower right, in that order.  Floating-point contraction is OFF for this file (the pragma below): a fused
// multiply-add of `s * 0.25f` into the next level's sum would keep the bits a denormal loses in the product, and
// the torch expression (pix2latent_amd.loss_functions.area_pool_torch) does not.  (The __fadd_rn / __fmul_rn of the
// HIP headers do not stop it: they are plain operators compiled under the headers' own contraction state.)  The
// result is that expression's, bit for bit, signed zeros included.
//
// Three launches, one thread per group of WD consecutive source floats of a source row block (WD = f, at least 4:
// 16-byte loads; 2 when f = 2 and W is no multiple of 4: 8-byte loads), no LDS, no atomics, no reduction across
// threads; nothing is allocated and nothing waits for the host:
//   pack     [B,3,H,W] -> pool_f -> [B,H/f,W/f,16], channels 3..15 written as +0.0; the source is read once
//   nchw     [B,C,H,W] (* mul) -> pool_f -> [B,C,H/f,W/f]
//   unpool   dout [B,3,H,W] = d_full16[...,0:3] + expand_f(d_small16[...,0:3]) * (1 / f^2); dout is written once,
//            one thread per 4 (2) consecutive pixels of a row
#include "p2l_common.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;

__device__ __forceinline__ float pool4(float a, float b, float c, float d) {
  return ((a + b) + (c + d)) * 0.25f;
}

template <int WD>
__device__ __forceinline__ void load_row(const float* p, float (&o)[WD]) {
  if constexpr (WD == 2) {
    const f32x2 v = *reinterpret_cast<const f32x2*>(p);
    o[0] = v.x;
    o[1] = v.y;
  } else {
#pragma unroll
    for (int j = 0; j < WD / 4; ++j) {
      const f32x4 v = reinterpret_cast<const f32x4*>(p)[j];
      o[4 * j] = v.x;
      o[4 * j + 1] = v.y;
      o[4 * j + 2] = v.z;
      o[4 * j + 3] = v.w;
    }
  }
}

// the pooled row of S source rows x WD source columns at p (row pitch W): WD / S values
template <int S, int WD, bool MUL>
struct Strip {
  static __device__ __forceinline__ void run(const float* p, const float* m, size_t W, float (&o)[WD / S]) {
    float a[2 * WD / S], b[2 * WD / S];
    Strip<S / 2, WD, MUL>::run(p, m, W, a);
    Strip<S / 2, WD, MUL>::run(p + (S / 2) * W, MUL ? m + (S / 2) * W : m, W, b);
#pragma unroll
    for (int j = 0; j < WD / S; ++j) o[j] = pool4(a[2 * j], a[2 * j + 1], b[2 * j], b[2 * j + 1]);
  }
};
template <int WD, bool MUL>
struct Strip<1, WD, MUL> {
  static __device__ __forceinline__ void run(const float* p, const float* m, size_t, float (&o)[WD]) {
    load_row<WD>(p, o);
    if constexpr (MUL) {
      float mm[WD];
      load_row<WD>(m, mm);
#pragma unroll
      for (int j = 0; j < WD; ++j) o[j] = o[j] * mm[j];
    }
  }
};

// thread -> (plane, pooled row, group of WD source columns)
struct PoolIdx {
  size_t plane;
  int y, g;
};
__device__ __forceinline__ bool pool_idx(size_t planes, int h, int groups, PoolIdx& I) {
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= planes * h * groups) return false;
  const size_t t = idx / groups;
  I.g = (int)(idx - t * groups);
  I.plane = t / h;
  I.y = (int)(t - I.plane * h);
  return true;
}

template <int F, int WD, bool MUL>
__global__ __launch_bounds__(kThreads) void area_pool_nchw_kernel(const float* __restrict__ src,
                                                                  const float* __restrict__ mul,
                                                                  float* __restrict__ dst, size_t planes, int H,
                                                                  int W) {
  PoolIdx I;
  if (!pool_idx(planes, H / F, W / WD, I)) return;
  const size_t off = (I.plane * H + (size_t)I.y * F) * W + (size_t)I.g * WD;
  float o[WD / F];
  Strip<F, WD, MUL>::run(src + off, MUL ? mul + off : mul, (size_t)W, o);
  float* d = dst + (I.plane * (H / F) + I.y) * (size_t)(W / F) + (size_t)I.g * (WD / F);
#pragma unroll
  for (int j = 0; j < WD / F; ++j) d[j] = o[j];
}

template <int F, int WD>
__global__ __launch_bounds__(kThreads) void area_pool3_to_nhwc16_kernel(const float* __restrict__ src,
                                                                        float* __restrict__ dst, size_t Bn, int H,
                                                                        int W) {
  PoolIdx I;
  if (!pool_idx(Bn, H / F, W / WD, I)) return;
  float o[3][WD / F];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t off = ((I.plane * 3 + c) * H + (size_t)I.y * F) * W + (size_t)I.g * WD;
    Strip<F, WD, false>::run(src + off, nullptr, (size_t)W, o[c]);
  }
  f32x4* d = reinterpret_cast<f32x4*>(dst + ((I.plane * (H / F) + I.y) * (size_t)(W / F) + (size_t)I.g * (WD / F)) * 16);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < WD / F; ++j) {
    const f32x4 v = {o[0][j], o[1][j], o[2][j], 0.f};
    d[4 * j] = v;
    d[4 * j + 1] = z;
    d[4 * j + 2] = z;
    d[4 * j + 3] = z;
  }
}

// one thread per V consecutive pixels of a full-resolution row
template <int F, int V>
__global__ __launch_bounds__(kThreads) void area_unpool16_add_nchw3_kernel(const float* __restrict__ d_small16,
                                                                           const float* __restrict__ d_full16,
                                                                           float* __restrict__ dout, size_t Bn,
                                                                           int H, int W) {
  const int groups = W / V;
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= Bn * H * groups) return;
  const size_t t = idx / groups;
  const int x0 = (int)(idx - t * groups) * V;
  const size_t b = t / H;
  const int y = (int)(t - b * H);
  constexpr float inv = 1.f / (float)(F * F);
  constexpr int NS = V > F ? V / F : 1;          // pooled pixels under the V full-resolution ones
  const float* sp = d_small16 + ((b * (H / F) + y / F) * (size_t)(W / F) + x0 / F) * 16;
  f32x4 s[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) s[j] = *reinterpret_cast<const f32x4*>(sp + 16 * j);
  float o[3][V];
  const float* fp = d_full16 ? d_full16 + (t * W + x0) * 16 : nullptr;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const f32x4 g = s[V > F ? j / F : 0];
    o[0][j] = g.x * inv;
    o[1][j] = g.y * inv;
    o[2][j] = g.z * inv;
    if (fp) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(fp + 16 * j);
      o[0][j] = a.x + o[0][j];
      o[1][j] = a.y + o[1][j];
      o[2][j] = a.z + o[2][j];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* d = dout + ((b * 3 + c) * H + y) * (size_t)W + x0;
    if constexpr (V == 4) {
      const f32x4 v = {o[c][0], o[c][1], o[c][2], o[c][3]};
      *reinterpret_cast<f32x4*>(d) = v;
    } else {
      const f32x2 v = {o[c][0], o[c][1]};
      *reinterpret_cast<f32x2*>(d) = v;
    }
  }
}

bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

// f in {2, 4, 8, 16} dividing H and W; the grid of `threads` threads fits
bool pool_shape_ok(int64_t planes, int H, int W, int f) {
  if (planes < 1 || H < 1 || W < 1) return false;
  if (f != 2 && f != 4 && f != 8 && f != 16) return false;
  if (H % f || W % f) return false;
  return planes * H * W / 2 < (int64_t)INT32_MAX * kThreads;     // (every grid here has at most one thread per 2 floats)
}

dim3 grid_for(size_t threads) { return dim3((unsigned)((threads + kThreads - 1) / kThreads)); }

}  // namespace

#define P2L_POOL_DISPATCH(CALL)                                  \
  switch (f) {                                                   \
    case 2: if (W % 4) { CALL(2, 2); } else { CALL(2, 4); } break; \
    case 4: CALL(4, 4); break;                                   \
    case 8: CALL(8, 8); break;                                   \
    default: CALL(16, 16); break;                                \
  }

extern "C" int p2l_area_pool3_to_nhwc16(const float* src, float* dst, int Bn, int H, int W, int f, void* stream) {
  if (!src || !dst || !aligned16(src) || !aligned16(dst) || !pool_shape_ok(3 * (int64_t)Bn, H, W, f))
    return P2L_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define CALL(F, WD)                                                                                                  \
  hipLaunchKernelGGL((area_pool3_to_nhwc16_kernel<F, WD>), grid_for((size_t)Bn * (H / F) * (W / WD)), dim3(kThreads), \
                     0, st, src, dst, (size_t)Bn, H, W)
  P2L_POOL_DISPATCH(CALL)
#undef CALL
  return p2l_check_launch();
}

extern "C" int p2l_area_pool_nchw(const float* src, const float* mul, float* dst, int Bn, int C, int H, int W, int f,
                                  void* stream) {
  if (!src || !dst || !aligned16(src) || !aligned16(mul) || !aligned16(dst) || Bn < 1 || C < 1 ||
      !pool_shape_ok((int64_t)Bn * C, H, W, f))
    return P2L_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const size_t planes = (size_t)Bn * C;
#define CALL(F, WD)                                                                                                   \
  do {                                                                                                                \
    const dim3 grid = grid_for(planes * (H / F) * (W / WD));                                                          \
    if (mul)                                                                                                          \
      hipLaunchKernelGGL((area_pool_nchw_kernel<F, WD, true>), grid, dim3(kThreads), 0, st, src, mul, dst, planes, H, \
                         W);                                                                                          \
    else                                                                                                              \
      hipLaunchKernelGGL((area_pool_nchw_kernel<F, WD, false>), grid, dim3(kThreads), 0, st, src, mul, dst, planes,   \
                         H, W);                                                                                       \
  } while (0)
  P2L_POOL_DISPATCH(CALL)
#undef CALL
  return p2l_check_launch();
}

extern "C" int p2l_area_unpool16_add_nchw3(const float* d_small16, const float* d_full16, float* dout, int Bn, int H,
                                           int W, int f, void* stream) {
  if (!d_small16 || !dout || !aligned16(d_small16) || !aligned16(d_full16) || !aligned16(dout) ||
      !pool_shape_ok(3 * (int64_t)Bn, H, W, f))
    return P2L_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define CALL(F, V)                                                                                                \
  hipLaunchKernelGGL((area_unpool16_add_nchw3_kernel<F, V>), grid_for((size_t)Bn * H * (W / V)), dim3(kThreads), 0, \
                     st, d_small16, d_full16, dout, (size_t)Bn, H, W)
  switch (f) {
    case 2: if (W % 4) { CALL(2, 2); } else { CALL(2, 4); } break;
    case 4: CALL(4, 4); break;
    case 8: CALL(8, 4); break;
    default: CALL(16, 4); break;
  }
#undef CALL
  return p2l_check_launch();
}
