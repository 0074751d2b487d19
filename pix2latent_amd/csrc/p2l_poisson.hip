// Poisson compositing of generated images into their target photograph (pix2latent/utils/image.py
// poisson_blend).  Per (image, channel):
//
//   Omega = the masked pixels that are not on the outermost one-pixel frame of the image
//   out   = target                                  outside Omega, bit for bit
//   out   = clamp(generated + u, -1, 1)             inside Omega
//   4 u(p) - sum_{q in N4(p), q in Omega} u(q) = sum_{q in N4(p), q not in Omega} (target(q) - generated(q))
//
// i.e. seamless cloning with the source's own gradients, written as a membrane correction u.  The
// system is SPD; it is solved by conjugate gradients with iterates, residual, search direction and
// every dot product in fp64.
//
// Form: ONE block of 1024 threads (16 waves) owns one system from start to finish.  It finds the
// bounding box of Omega, lays x, r and p out over the box plus a one-element halo of zeros (so the
// stencil reads its neighbours without a membership test: p is 0 wherever it is no unknown) and
// keeps the three arrays in LDS when they fit, in its slice of the workspace otherwise.  Wave w
// walks the rows w, w + 16, ... of the box, lane l the columns l, l + 64, ...: every thread owns the
// same elements in every phase, only the stencil reads of p cross threads, and those are separated
// from the writes of p by a block barrier (which also waits for the stores of the global form).
// A dot product is summed per thread in that walk's order, then over the wave by butterfly, then
// over the 16 wave partials in wave order by every thread: the sums, the step lengths and the
// iteration count depend on the box and its contents only, not on the batch or the system's place
// in it, and every thread sees the same values, so all leave the loop together.  No atomics, no
// grid barrier, no host synchronisation.
#include "p2l_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
// dynamic LDS a block may take for its state (the CU has 160 KB; the rest stays for the static part)
constexpr size_t kLdsStateBytes = 156 * 1024;

struct PoissonArgs {
  const float* target;
  const uint8_t* mask;
  const float* gen;
  float* out;
  int64_t t_bstride, m_bstride;   // elements between images; 0 = shared by the batch
  int C, H, W, max_iter;
  double tol;
  double* ws;
  int64_t ws_stride;              // doubles per system
  int32_t* iters;
  double* relres;
  int lds_doubles;                // doubles of dynamic LDS the launch carries
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the block, the same value in every thread; `s` must not be reused before the next barrier
__device__ __forceinline__ double block_sum_f64(double v, double* s, int lane, int wave) {
  v = wave_sum_f64(v);
  if (lane == 0) s[wave] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) t += s[i];
  return t;
}

__device__ __forceinline__ double stencil(const double* p, int j, int pw) {
  return 4.0 * p[j] - ((p[j - pw] + p[j - 1]) + (p[j + 1] + p[j + pw]));
}

__global__ __launch_bounds__(kThreads) void poisson_cg_kernel(PoissonArgs a) {
  extern __shared__ double s_state[];
  __shared__ double s_red[2][kWaves];
  __shared__ int s_box[kWaves][4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sys = blockIdx.x, b = sys / a.C, c = sys - b * a.C;
  const int H = a.H, W = a.W;
  const int64_t HW = (int64_t)H * W;
  const float* __restrict__ t = a.target + b * a.t_bstride + c * HW;
  const float* __restrict__ g = a.gen + (int64_t)sys * HW;
  const uint8_t* __restrict__ m = a.mask + b * a.m_bstride;
  float* __restrict__ o = a.out + (int64_t)sys * HW;

  // out = target outside Omega, and the bounding box of Omega
  int y0 = H, y1 = -1, x0 = W, x1 = -1;
  for (int y = wave; y < H; y += kWaves) {
    const bool yin = y > 0 && y < H - 1;
    for (int x = lane; x < W; x += 64) {
      const int64_t i = (int64_t)y * W + x;
      if (yin && x > 0 && x < W - 1 && m[i]) {
        y0 = min(y0, y), y1 = max(y1, y), x0 = min(x0, x), x1 = max(x1, x);
      } else {
        o[i] = t[i];
      }
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    y0 = min(y0, __shfl_xor(y0, s, 64)), y1 = max(y1, __shfl_xor(y1, s, 64));
    x0 = min(x0, __shfl_xor(x0, s, 64)), x1 = max(x1, __shfl_xor(x1, s, 64));
  }
  if (lane == 0) s_box[wave][0] = y0, s_box[wave][1] = y1, s_box[wave][2] = x0, s_box[wave][3] = x1;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    y0 = min(y0, s_box[i][0]), y1 = max(y1, s_box[i][1]);
    x0 = min(x0, s_box[i][2]), x1 = max(x1, s_box[i][3]);
  }
  if (y1 < 0) {                                       // empty Omega: out = target
    if (tid == 0) a.iters[sys] = 0, a.relres[sys] = 0.0;
    return;
  }

  const int bh = y1 - y0 + 1, bw = x1 - x0 + 1, pw = bw + 2;
  const int n_pad = (bh + 2) * pw;                    // <= H * W: the box lies inside the frame
  double* X = 3 * (int64_t)n_pad <= a.lds_doubles ? s_state : a.ws + (int64_t)sys * a.ws_stride;
  double* R = X + n_pad;
  double* P = R + n_pad;
  const uint8_t* __restrict__ mb = m + (int64_t)y0 * W + x0;      // the box's corner
  const float* __restrict__ tb = t + (int64_t)y0 * W + x0;
  const float* __restrict__ gb = g + (int64_t)y0 * W + x0;

  for (int j = tid; j < 3 * n_pad; j += kThreads) X[j] = 0.0;
  __syncthreads();

  // r = p = b: the Dirichlet data target - generated of the neighbours outside Omega
  double acc = 0.0;
  for (int y = wave; y < bh; y += kWaves) {
    for (int x = lane; x < bw; x += 64) {
      const int64_t i = (int64_t)y * W + x;
      if (!mb[i]) continue;
      const int gy = y0 + y, gx = x0 + x;
      double rhs = 0.0;
      // (a neighbour on the frame is never in Omega, whatever its mask byte says)
      if (gy - 1 < 1 || !mb[i - W]) rhs += (double)tb[i - W] - (double)gb[i - W];
      if (gx - 1 < 1 || !mb[i - 1]) rhs += (double)tb[i - 1] - (double)gb[i - 1];
      if (gx + 1 > W - 2 || !mb[i + 1]) rhs += (double)tb[i + 1] - (double)gb[i + 1];
      if (gy + 1 > H - 2 || !mb[i + W]) rhs += (double)tb[i + W] - (double)gb[i + W];
      const int j = (y + 1) * pw + x + 1;
      R[j] = rhs;
      P[j] = rhs;
      acc += rhs * rhs;
    }
  }
  const double bb = block_sum_f64(acc, s_red[1], lane, wave);
  const double thresh = a.tol * a.tol * bb;
  double rr = bb;
  int it = 0;
  if (bb > 0.0) {                                     // b = 0: u = 0 at once
    for (; it < a.max_iter; ++it) {
      if (rr <= thresh) break;
      acc = 0.0;
      for (int y = wave; y < bh; y += kWaves) {
        for (int x = lane; x < bw; x += 64) {
          if (!mb[(int64_t)y * W + x]) continue;
          const int j = (y + 1) * pw + x + 1;
          acc += P[j] * stencil(P, j, pw);
        }
      }
      const double pAp = block_sum_f64(acc, s_red[0], lane, wave);
      if (!(pAp > 0.0)) break;
      const double alpha = rr / pAp;
      acc = 0.0;
      for (int y = wave; y < bh; y += kWaves) {
        for (int x = lane; x < bw; x += 64) {
          if (!mb[(int64_t)y * W + x]) continue;
          const int j = (y + 1) * pw + x + 1;
          const double ap = stencil(P, j, pw);
          X[j] += alpha * P[j];
          const double rj = R[j] - alpha * ap;
          R[j] = rj;
          acc += rj * rj;
        }
      }
      const double rr_new = block_sum_f64(acc, s_red[1], lane, wave);   // (its barrier: every read of p is done)
      const double beta = rr_new / rr;
      rr = rr_new;
      for (int y = wave; y < bh; y += kWaves) {
        for (int x = lane; x < bw; x += 64) {
          if (!mb[(int64_t)y * W + x]) continue;
          const int j = (y + 1) * pw + x + 1;
          P[j] = R[j] + beta * P[j];
        }
      }
      __syncthreads();
    }
  }

  float* __restrict__ ob = o + (int64_t)y0 * W + x0;
  for (int y = wave; y < bh; y += kWaves) {
    for (int x = lane; x < bw; x += 64) {
      const int64_t i = (int64_t)y * W + x;
      if (!mb[i]) continue;
      const float v = (float)((double)gb[i] + X[(y + 1) * pw + x + 1]);
      ob[i] = fminf(fmaxf(v, -1.0f), 1.0f);
    }
  }
  if (tid == 0) {
    a.iters[sys] = it;
    a.relres[sys] = bb > 0.0 ? sqrt(rr / bb) : 0.0;
  }
}

bool poisson_sizes_ok(int Bn, int C, int H, int W) {
  if (Bn < 1 || C < 1 || H < 1 || W < 1) return false;
  return (int64_t)H * W <= (int64_t)0x7fffffff / 3 && (int64_t)Bn * C <= 0x7fffffff;
}

}  // namespace

extern "C" size_t p2l_poisson_blend_ws_bytes(int Bn, int C, int H, int W) {
  if (!poisson_sizes_ok(Bn, C, H, W)) return 0;
  return (size_t)Bn * C * 3 * H * W * sizeof(double);
}

extern "C" int p2l_poisson_blend(const float* target, int64_t target_bstride, const uint8_t* mask,
                                 int64_t mask_bstride, const float* generated, float* out, int Bn, int C, int H,
                                 int W, double tol, int max_iter, int32_t* iters, double* relres, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!target || !mask || !generated || !out || !iters || !relres || !poisson_sizes_ok(Bn, C, H, W))
    return P2L_EINVAL;
  const int64_t HW = (int64_t)H * W;
  if ((target_bstride != 0 && target_bstride < C * HW) || (mask_bstride != 0 && mask_bstride < HW)) return P2L_EINVAL;
  if (!(tol >= 0.0) || max_iter < 0) return P2L_EINVAL;
  const size_t need = p2l_poisson_blend_ws_bytes(Bn, C, H, W);
  if (!ws || ws_bytes < need) return P2L_EWS;
  PoissonArgs a;
  a.target = target, a.mask = mask, a.gen = generated, a.out = out;
  a.t_bstride = target_bstride, a.m_bstride = mask_bstride;
  a.C = C, a.H = H, a.W = W, a.max_iter = max_iter;
  a.tol = tol;
  a.ws = (double*)ws, a.ws_stride = 3 * HW;
  a.iters = iters, a.relres = relres;
  size_t lds = (size_t)3 * HW * sizeof(double);
  if (lds > kLdsStateBytes) lds = kLdsStateBytes;
  a.lds_doubles = (int)(lds / sizeof(double));
  // more dynamic LDS than a launch gets by default: the kernel is told once per process (a runtime that
  // needs no telling may refuse the attribute; the launch below reports what matters)
  static const bool told = [] {
    if (hipFuncSetAttribute((const void*)poisson_cg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kLdsStateBytes) != hipSuccess)
      (void)hipGetLastError();                        // (not left behind for the check of the launch)
    return true;
  }();
  (void)told;
  hipLaunchKernelGGL(poisson_cg_kernel, dim3(Bn * C), dim3(kThreads), lds, (hipStream_t)stream, a);
  return p2l_check_launch();
}
