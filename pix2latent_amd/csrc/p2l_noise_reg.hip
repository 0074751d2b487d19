// StyleGAN2 noise regulariser and per-layer noise normalisation (the projector's
// noise_regularize / noise_normalize_ on the reference's flat noise variable).
//
// noises [Bn][T] fp32, layer l = the res_l x res_l row-major map at offset sum_{j<l} res_j^2.  Level 0 of a layer is
// the map (side s_0 = res_l); while s_k > 8 level k+1 has side s_k / 2 and
//   n^{k+1}[y,x] = ((n^k[2y,2x] + n^k[2y,2x+1]) + (n^k[2y+1,2x] + n^k[2y+1,2x+1])) * 0.25f          (fp32)
// Per candidate and level, with wrap-around indices:  ax = mean n[y,x] n[y,x-1],  ay = mean n[y,x] n[y-1,x],
// R_b = sum over layers and levels of ax^2 + ay^2.  Products of fp32 values are exact in fp64, every sum is fp64.
//
// Work units.  A level of side s is cut into max(1, s^2 / 4096) ITEMS; every item leaves one fp64 partial pair in
// the workspace and a finish kernel adds a level's partials in item order: no atomics, no memset, and the order
// of every sum is a function of the layer sizes alone -- not of Bn, of the candidate's row or of the call.
//
// Launches (none depends on Bn; blockIdx.y is the candidate):
//   forward, 3:   pool    one block per 64 x 64 tile of level 0 (a whole map up to 64^2): the tile goes to LDS once,
//                         leaves its level-0 partial (the left / upper neighbours of its first column / row come from
//                         global memory) and every pooled level that lies inside the tile (down to tile side 1 or map
//                         side 8) to the workspace
//                 corr    one block per item of the levels >= 1, reading the pooled levels back (a third of T, warm in
//                         cache); the one level no tile can make -- side 8 of a 1024^2 map, a pixel of which spans
//                         2 x 2 tiles -- is pooled here from the 16^2 level, by the one block that owns it
//                 finish  one block per candidate: ax, ay of every level, then R_b
//   backward, 1:  one block per level-0 tile.  g^k = (2 / s_k^2)(ax (n[y,x-1] + n[y,x+1]) + ay (n[y-1,x] + n[y+1,x]))
//                 and the level-0 gradient is sum_k 4^-k g^k[y >> k, x >> k]: the block builds, coarsest level first,
//                 the running sum of the coarse terms over its own footprint in LDS (fp64, 1366 entries), then every
//                 pixel adds its level-0 term from a haloed LDS tile, scales by gloss[b] and rounds ONCE to fp32.
//   normalise, 3: sum -> squared deviations about the mean -> (n - mean) / std in place, items of 4096 floats,
//                 fp64, unbiased std; a constant map divides by zero as the torch expression does.
// Traffic per candidate: forward reads T once (+ halo) and writes / re-reads T / 3; backward reads T + T / 3 and
// writes T -- noises twice, dnoises once, the coarse levels from cache.
#include "p2l_common.h"

namespace {

constexpr int kThreads = 256;            // 4 waves
constexpr int kTile = 64;                // level-0 tile side
constexpr int kItemLog = 12;             // 4096 pixels per item
constexpr int kMaxLayers = 32;
constexpr int kMaxRes = 1024;            // one level beyond the tiles' reach at most (corr kernel, `tail`)
constexpr int kCoarse = 1408;            // >= 1024 + 256 + 64 + 16 + 4 + 1 + 1 running sums of a tile

struct NrLayer {
  int res;          // side of level 0
  int off0;         // float offset of the map in a row of noises
  int pool_off;     // float offset of level 1 in a candidate's pooled levels
  int lev_base;     // index of level 0 among the candidate's levels (layer-major, finest first)
  int item_base;    // index of the first item of level 0 among the candidate's items (same order)
  int tile_base;    // first block of the layer in the grids over level-0 items
  int blk2_base;    // first block of the layer in the grid over the items of the levels >= 1
};

struct NrPlan {
  int n_layers, n_levels, n_items, n_tiles, n_blk2;
  int T, P;         // floats per candidate: noises, pooled levels
  int pad;
  NrLayer L[kMaxLayers];
};

__host__ __device__ __forceinline__ int nr_items(int s) {
  const int n = (s * s) >> kItemLog;
  return n > 0 ? n : 1;
}
__host__ __device__ __forceinline__ int nr_nlev(int res) {
  int n = 1;
  for (int s = res; s > 8; s >>= 1) ++n;
  return n;
}

bool nr_make_plan(const int32_t* res, int n_layers, int Bn, NrPlan& p) {
  if (!res || n_layers < 1 || n_layers > kMaxLayers || Bn < 1 || Bn > 65535) return false;
  p = NrPlan();
  p.n_layers = n_layers;
  for (int l = 0; l < n_layers; ++l) {
    const int r = res[l];
    if (r < 4 || r > kMaxRes || !is_pow2(r)) return false;
    NrLayer& L = p.L[l];
    L.res = r;
    L.off0 = p.T;
    L.pool_off = p.P;
    L.lev_base = p.n_levels;
    L.item_base = p.n_items;
    L.tile_base = p.n_tiles;
    L.blk2_base = p.n_blk2;
    p.T += r * r;
    p.n_tiles += nr_items(r);
    const int nlev = nr_nlev(r);
    for (int k = 0; k < nlev; ++k) {
      const int s = r >> k;
      p.n_items += nr_items(s);
      if (k > 0) {
        p.P += s * s;
        p.n_blk2 += nr_items(s);
      }
    }
    p.n_levels += nlev;
  }
  return true;
}

// workspace: corr [Bn][n_levels][2] fp64 | partials [Bn][n_items][2] fp64 | pooled levels [Bn][P] fp32
struct NrWs {
  double* corr;
  double* part;
  float* pooled;
  size_t bytes;
};
NrWs nr_carve(const NrPlan& p, int Bn, void* ws) {
  NrWs w;
  const size_t nc = (size_t)Bn * p.n_levels * 2, np = (size_t)Bn * p.n_items * 2;
  w.bytes = (nc + np) * sizeof(double) + (size_t)Bn * p.P * sizeof(float);
  w.bytes = (w.bytes + 15) & ~(size_t)15;
  w.corr = w.part = nullptr;
  w.pooled = nullptr;
  if (ws) {
    w.corr = (double*)ws;
    w.part = w.corr + nc;
    w.pooled = (float*)(w.part + np);
  }
  return w;
}

bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sums of a and b over the block (wave butterflies, then the 4 waves in order) -> out[0], out[1]
__device__ __forceinline__ void block_sum2(double a, double b, double* red, double* out) {
  const int tid = threadIdx.x;
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = a;
    red[2 * (tid >> 6) + 1] = b;
  }
  __syncthreads();
  if (tid == 0) {
    out[0] = ((red[0] + red[2]) + red[4]) + red[6];
    out[1] = ((red[1] + red[3]) + red[5]) + red[7];
  }
}

// the layer a block of a grid over level-0 items belongs to
__device__ __forceinline__ int layer_of_tile(const NrPlan& p, int blk) {
  int l = 0;
  while (l + 1 < p.n_layers && p.L[l + 1].tile_base <= blk) ++l;
  return l;
}

__device__ __forceinline__ float pool4(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

__global__ __launch_bounds__(kThreads) void nr_pool_kernel(const float* __restrict__ noises, const NrPlan p,
                                                           float* __restrict__ pooled, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float lv[2][kTile * kTile];
  __shared__ double red[8];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int l = layer_of_tile(p, blockIdx.x);
  const NrLayer L = p.L[l];
  const int res = L.res, ts = res < kTile ? res : kTile, tpr = res / ts;
  const int ti = blockIdx.x - L.tile_base;
  const int ty0 = (ti / tpr) * ts, tx0 = (ti % tpr) * ts;
  const float* src = noises + (size_t)b * p.T + L.off0;

  const int q = ts >> 2;                                       // float4 per tile row
  for (int idx = tid; idx < ts * q; idx += kThreads) {
    const int y = idx / q, x = (idx - y * q) * 4;
    const float4 v = *(const float4*)(src + (size_t)(ty0 + y) * res + tx0 + x);
    *(float4*)&lv[0][y * ts + x] = v;
  }
  __syncthreads();

  // level 0: the pairs (pixel, left neighbour) and (pixel, upper neighbour) of the tile's own pixels
  double sx = 0.0, sy = 0.0;
  const int xl = (tx0 - 1) & (res - 1), yu = (ty0 - 1) & (res - 1);
  for (int idx = tid; idx < ts * ts; idx += kThreads) {
    const int y = idx / ts, x = idx & (ts - 1);
    const float c = lv[0][idx];
    const float le = x > 0 ? lv[0][idx - 1] : src[(size_t)(ty0 + y) * res + xl];
    const float up = y > 0 ? lv[0][idx - ts] : src[(size_t)yu * res + tx0 + x];
    sx += (double)c * (double)le;
    sy += (double)c * (double)up;
  }
  block_sum2(sx, sy, red, part + ((size_t)b * p.n_items + L.item_base + ti) * 2);

  // the pooled levels inside the tile
  float* dst = pooled + (size_t)b * p.P + L.pool_off;
  int cur = 0, cs = ts, s = res, k = 0;
  while (s > 8 && cs > 1) {
    const int ns = cs >> 1, S = s >> 1;
    ++k;
    const float* a = lv[cur];
    float* o = lv[cur ^ 1];
    const int oy = ty0 >> k, ox = tx0 >> k;
    for (int idx = tid; idx < ns * ns; idx += kThreads) {
      const int y = idx / ns, x = idx & (ns - 1);
      const float* r0 = a + (2 * y) * cs + 2 * x;
      const float v = pool4(r0[0], r0[1], r0[cs], r0[cs + 1]);
      o[idx] = v;
      dst[(size_t)(oy + y) * S + ox + x] = v;
    }
    __syncthreads();
    dst += S * S;
    cur ^= 1;
    cs = ns;
    s = S;
  }
}

__global__ __launch_bounds__(kThreads) void nr_corr_kernel(const NrPlan p, float* __restrict__ pooled,
                                                           double* __restrict__ part) {
  __shared__ float tail[64];
  __shared__ double red[8];
  const int tid = threadIdx.x, b = blockIdx.y;
  int l = 0;
  while (l + 1 < p.n_layers && p.L[l + 1].blk2_base <= (int)blockIdx.x) ++l;
  const NrLayer L = p.L[l];
  const int res = L.res;
  // level k >= 1 and item r of it
  int r = blockIdx.x - L.blk2_base, k = 1, item = L.item_base + nr_items(res);
  size_t off = (size_t)b * p.P + L.pool_off;
  for (;; ++k) {
    const int s_ = res >> k, n = nr_items(s_);
    if (r < n) break;
    r -= n;
    item += n;
    off += (size_t)s_ * s_;
  }
  const int s = res >> k;
  float* lvl = pooled + off;
  const float* src = lvl;
  if (s * kTile < res) {
    // beyond the tiles' reach (s = 8 of a 1024^2 map): pooled here from the level before it
    const float* prev = lvl - (size_t)(2 * s) * (2 * s);
    if (tid < s * s && tid < 64) {
      const int y = tid / s, x = tid & (s - 1);
      const float* r0 = prev + (2 * y) * (2 * s) + 2 * x;
      const float v = pool4(r0[0], r0[1], r0[2 * s], r0[2 * s + 1]);
      tail[tid] = v;
      lvl[tid] = v;
    }
    __syncthreads();
    src = tail;
  }
  const int n = s * s < (1 << kItemLog) ? s * s : (1 << kItemLog);
  const int base = r << kItemLog;
  double sx = 0.0, sy = 0.0;
  for (int idx = tid; idx < n; idx += kThreads) {
    const int pix = base + idx, y = pix / s, x = pix & (s - 1);
    const float c = src[pix];
    const float le = src[y * s + ((x - 1) & (s - 1))];
    const float up = src[((y - 1) & (s - 1)) * s + x];
    sx += (double)c * (double)le;
    sy += (double)c * (double)up;
  }
  block_sum2(sx, sy, red, part + ((size_t)b * p.n_items + item + r) * 2);
}

__global__ __launch_bounds__(kThreads) void nr_finish_kernel(const NrPlan p, const double* __restrict__ part,
                                                             double* __restrict__ corr_ws, double* __restrict__ corr_out,
                                                             float* __restrict__ loss) {
  __shared__ double term[kThreads];
  const int t = threadIdx.x, b = blockIdx.x;
  if (t < p.n_levels) {
    int l = 0;
    while (l + 1 < p.n_layers && p.L[l + 1].lev_base <= t) ++l;
    const int res = p.L[l].res, k = t - p.L[l].lev_base;
    int item = p.L[l].item_base;
    for (int j = 0; j < k; ++j) item += nr_items(res >> j);
    const int s = res >> k, n = nr_items(s);
    const double* pp = part + ((size_t)b * p.n_items + item) * 2;
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i < n; ++i) {
      sx += pp[2 * i];
      sy += pp[2 * i + 1];
    }
    const double inv = 1.0 / ((double)s * (double)s);
    const double ax = sx * inv, ay = sy * inv;
    const size_t o = ((size_t)b * p.n_levels + t) * 2;
    corr_ws[o] = ax;
    corr_ws[o + 1] = ay;
    if (corr_out) {
      corr_out[o] = ax;
      corr_out[o + 1] = ay;
    }
    term[t] = ax * ax + ay * ay;
  }
  __syncthreads();
  if (t == 0) {
    double R = 0.0;
    for (int i = 0; i < p.n_levels; ++i) R += term[i];
    loss[b] = (float)R;
  }
}

// LDS offset of the running sums of level k >= 1 of a tile of side ts
__device__ __forceinline__ int coarse_off(int ts, int k) {
  int o = 0;
  for (int j = 1; j < k; ++j) {
    const int rs = (ts >> j) > 0 ? (ts >> j) : 1;
    o += rs * rs;
  }
  return o;
}

__global__ __launch_bounds__(kThreads) void nr_bwd_kernel(const float* __restrict__ noises, const NrPlan p,
                                                          const float* __restrict__ pooled,
                                                          const double* __restrict__ corr,
                                                          const float* __restrict__ gloss, float* __restrict__ dn) {
  __shared__ float t0[(kTile + 2) * (kTile + 2)];
  __shared__ double cs[kCoarse];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int l = layer_of_tile(p, blockIdx.x);
  const NrLayer L = p.L[l];
  const int res = L.res, ts = res < kTile ? res : kTile, tpr = res / ts;
  const int ti = blockIdx.x - L.tile_base;
  const int ty0 = (ti / tpr) * ts, tx0 = (ti % tpr) * ts;
  const float* src = noises + (size_t)b * p.T + L.off0;
  const double* cr = corr + ((size_t)b * p.n_levels + L.lev_base) * 2;
  const int nlev = nr_nlev(res);

  // the tile with a one-pixel wrapped halo
  const int hs = ts + 2;
  for (int idx = tid; idx < hs * hs; idx += kThreads) {
    const int yy = idx / hs, xx = idx - yy * hs;
    const int gy = (ty0 + yy - 1) & (res - 1), gx = (tx0 + xx - 1) & (res - 1);
    t0[idx] = src[(size_t)gy * res + gx];
  }

  // running sums of the coarse terms over the tile's footprint, coarsest level first:
  // cs_k[Y,X] = 4^-k g^k[Y,X] + cs_{k+1}[Y >> 1, X >> 1]
  for (int k = nlev - 1; k >= 1; --k) {
    const int s = res >> k, rs = (ts >> k) > 0 ? (ts >> k) : 1;
    const int oy = ty0 >> k, ox = tx0 >> k;
    size_t off = (size_t)b * p.P + L.pool_off;
    for (int j = 1; j < k; ++j) off += (size_t)(res >> j) * (res >> j);
    const float* lvl = pooled + off;
    const double ax = cr[2 * k], ay = cr[2 * k + 1];
    const double w = ldexp(2.0 / ((double)s * (double)s), -2 * k);
    const int co = coarse_off(ts, k), co1 = coarse_off(ts, k + 1);
    const int rs1 = (ts >> (k + 1)) > 0 ? (ts >> (k + 1)) : 1;
    const int oy1 = ty0 >> (k + 1), ox1 = tx0 >> (k + 1);
    for (int idx = tid; idx < rs * rs; idx += kThreads) {
      const int Y = oy + idx / rs, X = ox + (idx & (rs - 1));
      const double le = lvl[Y * s + ((X - 1) & (s - 1))], ri = lvl[Y * s + ((X + 1) & (s - 1))];
      const double up = lvl[((Y - 1) & (s - 1)) * s + X], dw = lvl[((Y + 1) & (s - 1)) * s + X];
      double c = w * (ax * (le + ri) + ay * (up + dw));
      if (k + 1 < nlev) c += cs[co1 + ((Y >> 1) - oy1) * rs1 + ((X >> 1) - ox1)];
      cs[co + idx] = c;
    }
    __syncthreads();
  }
  __syncthreads();                                             // (the halo tile, when there was no coarse level)

  const double ax = cr[0], ay = cr[1];
  const double w = 2.0 / ((double)res * (double)res);
  const double gl = gloss ? (double)gloss[b] : 1.0;
  float* dst = dn + (size_t)b * p.T + L.off0;
  const int q = ts >> 2, hts = ts >> 1;
  for (int idx = tid; idx < ts * q; idx += kThreads) {
    const int y = idx / q, x = (idx - y * q) * 4;
    const float* c0 = t0 + (y + 1) * hs + x + 1;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double le = c0[j - 1], ri = c0[j + 1], up = c0[j - hs], dw = c0[j + hs];
      double g = w * (ax * (le + ri) + ay * (up + dw));
      if (nlev > 1) g += cs[(y >> 1) * hts + ((x + j) >> 1)];
      o[j] = (float)(g * gl);
    }
    *(float4*)(dst + (size_t)(ty0 + y) * res + tx0 + x) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- per-layer normalisation: block = item `it` of layer l (4096 consecutive floats, a whole map up to 64^2) ----
struct NrItem {
  float* x;          // the item's floats
  int n;             // how many
  int n_items;       // items of the layer
  int count;         // floats of the layer
  double* part;      // the layer's partial pairs, [n_items][2]
  int it;
};
__device__ __forceinline__ NrItem nr_item(const NrPlan& p, float* noises, double* part) {
  const int b = blockIdx.y, l = layer_of_tile(p, blockIdx.x);
  const NrLayer L = p.L[l];
  NrItem I;
  I.it = blockIdx.x - L.tile_base;
  I.count = L.res * L.res;
  I.n = I.count < (1 << kItemLog) ? I.count : (1 << kItemLog);
  I.n_items = nr_items(L.res);
  I.x = noises + (size_t)b * p.T + L.off0 + ((size_t)I.it << kItemLog);
  I.part = part + ((size_t)b * p.n_items + L.item_base) * 2;
  return I;
}
// sum of member `m` of the layer's partials in item order, to every thread
__device__ __forceinline__ double nr_layer_sum(const NrItem& I, int m, double* bc) {
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < I.n_items; ++i) t += I.part[2 * i + m];
    *bc = t;
  }
  __syncthreads();
  return *bc;
}

__global__ __launch_bounds__(kThreads) void nr_norm_sum_kernel(float* __restrict__ noises, const NrPlan p,
                                                               double* __restrict__ part) {
  __shared__ double red[8];
  const NrItem I = nr_item(p, noises, part);
  double t = 0.0;
  for (int idx = threadIdx.x; idx < (I.n >> 2); idx += kThreads) {
    const float4 v = ((const float4*)I.x)[idx];
    t += (((double)v.x + (double)v.y) + (double)v.z) + (double)v.w;
  }
  t = wave_sum_f64(t);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) I.part[2 * I.it] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kThreads) void nr_norm_dev_kernel(float* __restrict__ noises, const NrPlan p,
                                                               double* __restrict__ part) {
  __shared__ double red[8];
  __shared__ double bc;
  const NrItem I = nr_item(p, noises, part);
  const double mean = nr_layer_sum(I, 0, &bc) / (double)I.count;
  double t = 0.0;
  for (int idx = threadIdx.x; idx < (I.n >> 2); idx += kThreads) {
    const float4 v = ((const float4*)I.x)[idx];
    const double a = (double)v.x - mean, b_ = (double)v.y - mean, c = (double)v.z - mean, d = (double)v.w - mean;
    t += ((a * a + b_ * b_) + c * c) + d * d;
  }
  t = wave_sum_f64(t);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) I.part[2 * I.it + 1] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kThreads) void nr_norm_apply_kernel(float* __restrict__ noises, const NrPlan p,
                                                                 double* __restrict__ part) {
  __shared__ double bc[2];
  const NrItem I = nr_item(p, noises, part);
  const double mean = nr_layer_sum(I, 0, &bc[0]) / (double)I.count;
  const double sd = sqrt(nr_layer_sum(I, 1, &bc[1]) / (double)(I.count - 1));
  for (int idx = threadIdx.x; idx < (I.n >> 2); idx += kThreads) {
    float4 v = ((const float4*)I.x)[idx];
    v.x = (float)(((double)v.x - mean) / sd);
    v.y = (float)(((double)v.y - mean) / sd);
    v.z = (float)(((double)v.z - mean) / sd);
    v.w = (float)(((double)v.w - mean) / sd);
    ((float4*)I.x)[idx] = v;
  }
}

}  // namespace

extern "C" size_t p2l_sg2_noise_reg_ws_bytes(const int32_t* res, int n_layers, int Bn) {
  NrPlan p;
  if (!nr_make_plan(res, n_layers, Bn, p)) return 0;
  return nr_carve(p, Bn, nullptr).bytes;
}

extern "C" int p2l_sg2_noise_reg_fwd(const float* noises, const int32_t* res, int n_layers, int Bn, float* loss,
                                     double* corr, void* ws, size_t ws_bytes, void* stream) {
  NrPlan p;
  if (!noises || !loss || !aligned16(noises) || !nr_make_plan(res, n_layers, Bn, p)) return P2L_EINVAL;
  const NrWs w = nr_carve(p, Bn, ws);
  if (!ws || !aligned16(ws) || ws_bytes < w.bytes) return P2L_EWS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nr_pool_kernel, dim3(p.n_tiles, Bn), dim3(kThreads), 0, st, noises, p, w.pooled, w.part);
  if (p.n_blk2 > 0)
    hipLaunchKernelGGL(nr_corr_kernel, dim3(p.n_blk2, Bn), dim3(kThreads), 0, st, p, w.pooled, w.part);
  hipLaunchKernelGGL(nr_finish_kernel, dim3(Bn), dim3(kThreads), 0, st, p, w.part, w.corr, corr, loss);
  return p2l_check_launch();
}

extern "C" int p2l_sg2_noise_reg_bwd(const float* noises, const int32_t* res, int n_layers, int Bn,
                                     const float* gloss, float* dnoises, const void* ws, size_t ws_bytes,
                                     void* stream) {
  NrPlan p;
  if (!noises || !dnoises || !aligned16(noises) || !aligned16(dnoises) || !nr_make_plan(res, n_layers, Bn, p))
    return P2L_EINVAL;
  const NrWs w = nr_carve(p, Bn, const_cast<void*>(ws));
  if (!ws || !aligned16(ws) || ws_bytes < w.bytes) return P2L_EWS;
  hipLaunchKernelGGL(nr_bwd_kernel, dim3(p.n_tiles, Bn), dim3(kThreads), 0, (hipStream_t)stream, noises, p, w.pooled,
                     w.corr, gloss, dnoises);
  return p2l_check_launch();
}

extern "C" int p2l_sg2_noise_normalize(float* noises, const int32_t* res, int n_layers, int Bn, void* ws,
                                       size_t ws_bytes, void* stream) {
  NrPlan p;
  if (!noises || !aligned16(noises) || !nr_make_plan(res, n_layers, Bn, p)) return P2L_EINVAL;
  const NrWs w = nr_carve(p, Bn, ws);
  if (!ws || !aligned16(ws) || ws_bytes < w.bytes) return P2L_EWS;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.n_tiles, Bn);
  hipLaunchKernelGGL(nr_norm_sum_kernel, grid, dim3(kThreads), 0, st, noises, p, w.part);
  hipLaunchKernelGGL(nr_norm_dev_kernel, grid, dim3(kThreads), 0, st, noises, p, w.part);
  hipLaunchKernelGGL(nr_norm_apply_kernel, grid, dim3(kThreads), 0, st, noises, p, w.part);
  return p2l_check_launch();
}
