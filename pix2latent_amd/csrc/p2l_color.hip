// Colour transformations of the reference (pix2latent/transform/color_transform.py): a chain of
// hue / gamma / saturation / brightness / contrast ops on NCHW fp32 RGB images in [-1, 1],
// bit-exact to torchvision's PIL path at 8-bit precision ("colour").
//
// Per op and pixel the reference does: k = byte(((x + 1) / 2) * 255)  (fp32, truncation, wraps
// modulo 256), the Pillow integer op on k, then y = 2 * (k / 255 - 0.5) in fp32.  Between two
// chained ops the bytes go through that float and back again; the round trip is not always the
// identity, so it is kept (as a 256-entry table).
//
// One thread owns a group of 4 consecutive pixels (one float4 per channel plane) when the plane is
// a multiple of 4 floats and both pointers are 16-byte aligned, else 1 pixel.  A block covers one
// image (blockIdx.y), so every per-image value (op parameters, gamma LUTs, contrast means) is
// staged once in LDS.  The chain is one launch; each contrast op adds one pre-pass over the image
// that recomputes the chain up to it and sums its L image per image with 64-bit integer atomics
// (exact, order-independent), into a workspace the entry point zeroes first.
//
// No contraction anywhere: the reference's arithmetic is fp32 / fp64 without FMA.
#include "p2l_common.h"

namespace {

#pragma clang fp contract(off)

constexpr int kThreads = 256;

struct ColorArgs {
  int n_ops;        // ops applied (the main pass: all; a pre-pass: the ops before its contrast op)
  int sum_slot;     // pre-pass: workspace slot of the sums it produces; -1: the main pass
  int op[P2L_COLOR_MAX_OPS];
  int slot[P2L_COLOR_MAX_OPS];                 // contrast ops: workspace slot of their L sums
  const float* param[P2L_COLOR_MAX_OPS];
  const uint8_t* lut[P2L_COLOR_MAX_OPS];       // gamma ops: [Bn][256]
};

// ((x + 1) / 2) * 255 in fp32, then torch's float -> uint8: truncation through int64, modulo 256
__device__ __forceinline__ int to_byte(float x) {
  const float v = ((x + 1.0f) / 2.0f) * 255.0f;
  return (int)((long long)v & 255);
}

// to_tensor (fp32 k / 255, correctly rounded) then 2 * (y - 0.5)
__device__ __forceinline__ float from_byte(int k) { return 2.0f * ((float)k / 255.0f - 0.5f); }

__device__ __forceinline__ int luma(int r, int g, int b) {      // PIL convert('L')
  return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;
}

// PIL Image.blend(deg, img, alpha), alpha fp32: deg + alpha * (img - deg) in fp32, truncated;
// outside [0, 1] the value is clipped to [0, 255] first
__device__ __forceinline__ int blend(int deg, int img, float alpha, bool inside) {
  const float v = (float)deg + alpha * (float)(img - deg);
  if (inside) return (int)v;
  return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)v);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// PIL convert('HSV') (Convert.c rgb2hsv), the hue shifted by `shift` modulo 256, then convert('RGB')
// (hsv2rgb).  Float where Pillow is float, double where its constants promote.
__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = maxc;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr;
    const float gc = (float)(maxc - g) / cr;
    const float bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    // fmod(h / 6 + 1, 1): the argument lies in (0, 2), and x - 1 is exact on [1, 2]
    const double x = (double)h / 6.0 + 1.0;
    h = (float)(x >= 1.0 ? x - 1.0 : x);
    uh = clip8((int)((double)h * 255.0));
    us = clip8((int)((double)s * 255.0));
  }
  uh = (uh + shift) & 255;
  if (us == 0) {
    r = g = b = uv;
    return;
  }
  const double h6 = (double)(float)uh * 6.0 / 255.0;
  const int i = (int)floor(h6);
  const float f = (float)(h6 - (double)i);
  const float fs = (float)((double)(float)us / 255.0);
  const double v = (double)(float)uv;
  const int p = clip8((int)round(v * (1.0 - (double)fs)));
  const int q = clip8((int)round(v * (1.0 - (double)(fs * f))));
  const int t = clip8((int)round(v * (1.0 - (double)fs * (1.0 - (double)f))));
  switch (i % 6) {
    case 0: r = uv; g = t; b = p; break;
    case 1: r = q; g = uv; b = p; break;
    case 2: r = p; g = uv; b = t; break;
    case 3: r = p; g = q; b = uv; break;
    case 4: r = t; g = p; b = uv; break;
    default: r = uv; g = p; b = q; break;
  }
}

struct Staged {
  float y[256];                                 // k -> 2 * (k / 255 - 0.5)
  uint8_t rt[256];                              // k -> byte(y(k)): the float round trip between two ops
  uint8_t lut[P2L_COLOR_MAX_OPS][256];          // gamma ops
  float alpha[P2L_COLOR_MAX_OPS];               // blend factor (fp32 t) / hue shift / contrast mean
  int ival[P2L_COLOR_MAX_OPS];
  unsigned long long red[kThreads / 64];
};

__device__ __forceinline__ void apply_op(const Staged& s, int j, int op, int& r, int& g, int& b) {
  const float a = s.alpha[j];
  const bool inside = a >= 0.0f && a <= 1.0f;
  switch (op) {
    case P2L_COLOR_BRIGHTNESS:
      r = blend(0, r, a, inside); g = blend(0, g, a, inside); b = blend(0, b, a, inside);
      break;
    case P2L_COLOR_SATURATION: {
      const int L = luma(r, g, b);
      r = blend(L, r, a, inside); g = blend(L, g, a, inside); b = blend(L, b, a, inside);
      break;
    }
    case P2L_COLOR_CONTRAST: {
      const int m = s.ival[j];
      r = blend(m, r, a, inside); g = blend(m, g, a, inside); b = blend(m, b, a, inside);
      break;
    }
    case P2L_COLOR_GAMMA:
      r = s.lut[j][r]; g = s.lut[j][g]; b = s.lut[j][b];
      break;
    default:
      hue_shift(r, g, b, s.ival[j]);
      break;
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void color_kernel(const float* src, float* dst, ColorArgs A, int HW,
                                                         unsigned long long* sums) {
  __shared__ Staged s;
  const int bimg = blockIdx.y, tid = threadIdx.x;
  s.y[tid] = from_byte(tid);
  s.rt[tid] = (uint8_t)to_byte(from_byte(tid));
  for (int j = 0; j < A.n_ops; ++j) {
    if (A.op[j] == P2L_COLOR_GAMMA) s.lut[j][tid] = A.lut[j][(size_t)bimg * 256 + tid];
  }
  if (tid < A.n_ops) {
    const int j = tid;
    const float p = A.param[j][bimg];
    s.alpha[j] = p;
    s.ival[j] = 0;
    if (A.op[j] == P2L_COLOR_HUE) {
      s.ival[j] = (int)((double)p * 255.0) & 255;       // np.array(f * 255).astype(np.uint8)
    } else if (A.op[j] == P2L_COLOR_CONTRAST) {         // ImageEnhance.Contrast: int(mean(L) + 0.5)
      const unsigned long long S = sums[(size_t)A.slot[j] * gridDim.y + bimg];
      s.ival[j] = (int)((double)S / (double)HW + 0.5);
    }
  }
  __syncthreads();

  const size_t plane = (size_t)HW;
  const size_t base = (size_t)bimg * 3 * plane;
  const int ngroups = HW / VEC;
  unsigned int lsum = 0;
  for (int gi = blockIdx.x * kThreads + tid; gi < ngroups; gi += gridDim.x * kThreads) {
    const size_t o = base + (size_t)gi * VEC;
    float x[3][VEC];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4*>(src + o + c * plane);
        x[c][0] = v.x; x[c][1] = v.y; x[c][2] = v.z; x[c][3] = v.w;
      } else {
        x[c][0] = src[o + c * plane];
      }
    }
    int k[3][VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      int r = to_byte(x[0][e]), g = to_byte(x[1][e]), b = to_byte(x[2][e]);
      for (int j = 0; j < A.n_ops; ++j) {
        if (j > 0) { r = s.rt[r]; g = s.rt[g]; b = s.rt[b]; }
        apply_op(s, j, A.op[j], r, g, b);
      }
      if (A.sum_slot >= 0) {
        if (A.n_ops > 0) { r = s.rt[r]; g = s.rt[g]; b = s.rt[b]; }
        lsum += (unsigned int)luma(r, g, b);
      }
      k[0][e] = r; k[1][e] = g; k[2][e] = b;
    }
    if (A.sum_slot < 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if constexpr (VEC == 4) {
          *reinterpret_cast<float4*>(dst + o + c * plane) =
              make_float4(s.y[k[c][0]], s.y[k[c][1]], s.y[k[c][2]], s.y[k[c][3]]);
        } else {
          dst[o + c * plane] = s.y[k[c][0]];
        }
      }
    }
  }
  if (A.sum_slot >= 0) {
    unsigned long long v = lsum;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) s.red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
      const unsigned long long t = (s.red[0] + s.red[1]) + (s.red[2] + s.red[3]);
      atomicAdd(&sums[(size_t)A.sum_slot * gridDim.y + bimg], t);
    }
  }
}

int n_contrast(const P2LColorChain* ch) {
  int n = 0;
  for (int j = 0; j < ch->n_ops; ++j) n += ch->ops[j].op == P2L_COLOR_CONTRAST;
  return n;
}

bool chain_ok(const P2LColorChain* ch) {
  if (!ch || ch->size < sizeof(P2LColorChain) || ch->n_ops < 1 || ch->n_ops > P2L_COLOR_MAX_OPS) return false;
  for (int j = 0; j < ch->n_ops; ++j) {
    const P2LColorOp& o = ch->ops[j];
    if (o.op < P2L_COLOR_BRIGHTNESS || o.op > P2L_COLOR_HUE || !o.param) return false;
    if (o.op == P2L_COLOR_GAMMA && !o.lut) return false;
  }
  return true;
}

}  // namespace

extern "C" size_t p2l_color_adjust_ws_bytes(const P2LColorChain* chain, int Bn) {
  if (!chain_ok(chain) || Bn < 1) return 0;
  return (size_t)n_contrast(chain) * Bn * sizeof(unsigned long long);
}

extern "C" int p2l_color_adjust(const P2LColorChain* chain, const float* src, float* dst, int Bn, int C, int H,
                                int W, void* workspace, size_t ws_bytes, void* stream) {
  if (!chain_ok(chain) || !src || !dst || Bn < 1 || Bn > 65535 || C != 3 || H < 1 || W < 1) return P2L_EINVAL;
  if ((long long)H * W > (1LL << 30)) return P2L_EINVAL;
  const size_t need = p2l_color_adjust_ws_bytes(chain, Bn);
  if (need && (!workspace || ws_bytes < need)) return P2L_EWS;
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  const bool vec = HW % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const int ngroups = vec ? HW / 4 : HW;
  // enough blocks to fill the device (~8k in flight over all images), a grid-stride loop beyond
  const int cap = Bn >= 8192 ? 1 : 8192 / Bn, want = cdiv(ngroups, kThreads);
  const int nblk = want < cap ? want : cap;
  const dim3 grid(nblk, Bn);
  unsigned long long* sums = (unsigned long long*)workspace;

  ColorArgs A{};
  int slot = 0;
  for (int j = 0; j < chain->n_ops; ++j) {
    A.op[j] = chain->ops[j].op;
    A.param[j] = chain->ops[j].param;
    A.lut[j] = chain->ops[j].lut;
    A.slot[j] = A.op[j] == P2L_COLOR_CONTRAST ? slot++ : -1;
  }
  if (need) {
    const hipError_t e = hipMemsetAsync(workspace, 0, need, st);
    if (e != hipSuccess) {
      g_p2l_last_hip_error = (int)e;
      return P2L_ELAUNCH;
    }
    for (int j = 0; j < chain->n_ops; ++j) {
      if (A.op[j] != P2L_COLOR_CONTRAST) continue;
      ColorArgs P = A;
      P.n_ops = j;
      P.sum_slot = A.slot[j];
      if (vec) hipLaunchKernelGGL(color_kernel<4>, grid, dim3(kThreads), 0, st, src, dst, P, HW, sums);
      else hipLaunchKernelGGL(color_kernel<1>, grid, dim3(kThreads), 0, st, src, dst, P, HW, sums);
    }
  }
  A.n_ops = chain->n_ops;
  A.sum_slot = -1;
  if (vec) hipLaunchKernelGGL(color_kernel<4>, grid, dim3(kThreads), 0, st, src, dst, A, HW, sums);
  else hipLaunchKernelGGL(color_kernel<1>, grid, dim3(kThreads), 0, st, src, dst, A, HW, sums);
  return p2l_check_launch();
}
