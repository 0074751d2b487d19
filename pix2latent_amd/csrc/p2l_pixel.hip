// Weighted L2 pixel term of the projection loss (the StyleGAN2 projector's MSE term).
//
//   loss[b]   = sum_{c,p} w (t - o)^2 / wsum[b]                 w = weight * loss_mask, wsum from p2l_weight_sum
//   d[b,p,c]  = (gscale[b] / wsum[b]) * 2 * w * (o - t)
// o is the [B, H*W, 16] pixel-padded image (channels in floats 0..2), target / weight / loss_mask are [B,3,H,W].
//
// Memory-bound.  A block of 256 threads owns 1024 consecutive pixels and reads them in the shape each operand likes:
//   planes   thread i takes pixels 4i .. 4i+3 of the block: one 16-byte load per plane and channel where H*W is a
//            multiple of 4 (and the planes are 16-byte aligned), four 4-byte loads with a bounds test each otherwise;
//            w * m and t go to LDS (24 KB), and that is all the two forms differ in;
//   pixels   thread i then takes pixels i, i + 256, i + 512, i + 768 of the block: the 64 lanes of a wave read (and
//            the backward writes) 64 consecutive 64-byte pixels, as the L1 kernels do, and read w * m and t back from
//            consecutive LDS words.
// (Four consecutive pixels per thread for the image too -- the first form of this file -- left a wave's loads and
// stores 256 bytes apart per lane: 0.61 ms against the L1 kernels' 0.41 ms on nine 1024^2 images.)
//
// Forward, no atomics: a thread adds its 12 terms pixel by pixel, channel by channel; the block sums them with wave
// shuffles and four LDS slots and writes partial[b][block]; p2l_reduce_rows adds a sample's cdiv(H*W, 1024) partials
// in its own fixed order and divides by wsum[b].  The order depends on (H, W) alone: a sample's bits do not depend on
// the batch it sits in or on the stream it runs on.
#include "p2l_common.h"

#define ST(s) ((hipStream_t)(s))

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                         // consecutive pixels per thread
constexpr int kBlockPix = kThreads * kPix;

// floats p0 .. p0+3 of a plane; without VEC those at or past `end` read as 0
template <bool VEC>
__device__ __forceinline__ void load_plane4(const float* plane, size_t p0, size_t end, float (&o)[kPix]) {
  if constexpr (VEC) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(plane + p0);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < kPix; ++j) o[j] = (p0 + j < end) ? plane[p0 + j] : 0.f;
  }
}

// w * m and t of channel c for the thread's four pixels (a pixel past the end: w = 0, t = 0)
template <bool VEC>
__device__ __forceinline__ void load_wt(const float* target, const float* weight, const float* mask, size_t base,
                                        size_t p0, size_t HW, float (&w)[kPix], float (&t)[kPix]) {
  load_plane4<VEC>(weight + base, p0, HW, w);
  if (mask) {
    float m[kPix];
    load_plane4<VEC>(mask + base, p0, HW, m);
#pragma unroll
    for (int j = 0; j < kPix; ++j) w[j] *= m[j];
  }
  load_plane4<VEC>(target + base, p0, HW, t);
}

// w * m and t of the block's 1024 pixels into LDS, [channel][pixel of the block]; pixels past the end: 0
template <bool VEC>
__device__ __forceinline__ void stage_planes(const float* target, const float* weight, const float* mask, int b,
                                             size_t HW, size_t block0, float (*wm)[kBlockPix],
                                             float (*tt)[kBlockPix]) {
  const int q = threadIdx.x * kPix;
  const size_t p0 = block0 + q;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float w[kPix] = {0.f, 0.f, 0.f, 0.f}, t[kPix] = {0.f, 0.f, 0.f, 0.f};
    if (p0 < HW) load_wt<VEC>(target, weight, mask, ((size_t)b * 3 + c) * HW, p0, HW, w, t);
    *reinterpret_cast<f32x4*>(&wm[c][q]) = f32x4{w[0], w[1], w[2], w[3]};
    *reinterpret_cast<f32x4*>(&tt[c][q]) = f32x4{t[0], t[1], t[2], t[3]};
  }
  __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void l2_fwd_kernel(const float* __restrict__ img16,
                                                          const float* __restrict__ target,
                                                          const float* __restrict__ weight,
                                                          const float* __restrict__ mask,
                                                          float* __restrict__ partial, int HWi) {
  __shared__ __attribute__((aligned(16))) float wm[3][kBlockPix], tt[3][kBlockPix];
  __shared__ float red[4];
  const size_t HW = (size_t)HWi;
  const int b = blockIdx.y, nblk = gridDim.x;
  const size_t block0 = (size_t)blockIdx.x * kBlockPix;
  stage_planes<VEC>(target, weight, mask, b, HW, block0, wm, tt);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    const int q = j * kThreads + threadIdx.x;
    const size_t p = block0 + q;
    if (p < HW) {
      const f32x4 o = *reinterpret_cast<const f32x4*>(img16 + ((size_t)b * HW + p) * 16);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float d = tt[c][q] - o[c];
        acc += wm[c][q] * (d * d);
      }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)b * nblk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void l2_bwd_kernel(const float* __restrict__ img16,
                                                          const float* __restrict__ target,
                                                          const float* __restrict__ weight,
                                                          const float* __restrict__ mask,
                                                          const float* __restrict__ wsum,
                                                          const float* __restrict__ gscale, float* dimg16, int HWi,
                                                          int accumulate) {
  __shared__ __attribute__((aligned(16))) float wm[3][kBlockPix], tt[3][kBlockPix];
  const size_t HW = (size_t)HWi;
  const int b = blockIdx.y;
  const size_t block0 = (size_t)blockIdx.x * kBlockPix;
  const float gs = (gscale[b] / wsum[b]) * 2.f;
  stage_planes<VEC>(target, weight, mask, b, HW, block0, wm, tt);
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    const int q = j * kThreads + threadIdx.x;
    const size_t p = block0 + q;
    if (p < HW) {
      const size_t pix = (size_t)b * HW + p;
      const f32x4 o = *reinterpret_cast<const f32x4*>(img16 + pix * 16);
      f32x4 d = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 3; ++c) d[c] = (gs * wm[c][q]) * (o[c] - tt[c][q]);
      f32x4* dp = reinterpret_cast<f32x4*>(dimg16 + pix * 16);
      if (accumulate) {
        dp[0] = dp[0] + d;
      } else {
        const f32x4 z = {0, 0, 0, 0};
        dp[0] = d; dp[1] = z; dp[2] = z; dp[3] = z;
      }
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 16-byte plane loads: every plane of every sample starts on a 16-byte boundary
inline bool planes_vec(const float* target, const float* weight, const float* mask, int HW) {
  return HW % 4 == 0 && aligned16(target) && aligned16(weight) && aligned16(mask);
}

inline bool bad_shape(int Bn, int H, int W) {
  return Bn < 1 || Bn > 65535 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffLL;      // (Bn is the grid's y)
}

}  // namespace

extern "C" int p2l_l2_loss_nblk(int H, int W) {
  if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffLL) return 0;
  return cdiv((int64_t)H * W, kBlockPix);
}

extern "C" int p2l_l2_loss_fwd(const float* img16, const float* target, const float* weight,
                               const float* loss_mask, const float* wsum, float* loss, float* partial, int Bn,
                               int H, int W, void* stream) {
  if (!img16 || !target || !weight || !wsum || !loss || !partial) return P2L_EINVAL;
  if (bad_shape(Bn, H, W)) return P2L_EINVAL;
  const int HW = H * W, nblk = cdiv(HW, kBlockPix);
  if (planes_vec(target, weight, loss_mask, HW))
    hipLaunchKernelGGL(l2_fwd_kernel<true>, dim3(nblk, Bn), dim3(kThreads), 0, ST(stream), img16, target, weight,
                       loss_mask, partial, HW);
  else
    hipLaunchKernelGGL(l2_fwd_kernel<false>, dim3(nblk, Bn), dim3(kThreads), 0, ST(stream), img16, target, weight,
                       loss_mask, partial, HW);
  const int rc = p2l_check_launch();
  if (rc != P2L_OK) return rc;
  return p2l_reduce_rows(partial, loss, Bn, nblk, 1.f, wsum, 0, stream);
}

extern "C" int p2l_l2_loss_bwd(const float* img16, const float* target, const float* weight,
                               const float* loss_mask, const float* wsum, const float* gscale, float* dimg16,
                               int Bn, int H, int W, int accumulate, void* stream) {
  if (!img16 || !target || !weight || !wsum || !gscale || !dimg16) return P2L_EINVAL;
  if (bad_shape(Bn, H, W)) return P2L_EINVAL;
  const int HW = H * W, nblk = cdiv(HW, kBlockPix);
  if (planes_vec(target, weight, loss_mask, HW))
    hipLaunchKernelGGL(l2_bwd_kernel<true>, dim3(nblk, Bn), dim3(kThreads), 0, ST(stream), img16, target, weight,
                       loss_mask, wsum, gscale, dimg16, HW, accumulate);
  else
    hipLaunchKernelGGL(l2_bwd_kernel<false>, dim3(nblk, Bn), dim3(kThreads), 0, ST(stream), img16, target, weight,
                       loss_mask, wsum, gscale, dimg16, HW, accumulate);
  return p2l_check_launch();
}
