// fp64 Gram of a tall fp32 panel of up to 512 columns: G = X^T X ([cols][cols]) and the column sums of X,
// the O(rows) work of the StyleGAN2 GANSpace components (pix2latent_amd/edit/ganspace.py w_covariance,
// DESIGN.md section 9).  The 128-column kernel (p2l_edit.hip) is untouched; this is its wide sibling.
//
// X has `rows` rows and 1 <= cols <= 512 columns, element (r, j) at X[r * ld + j].  Products of fp32
// operands are exact in fp64; v_mfma_f64_16x16x4_f64 sums them.
//
// The columns form np = ceil(cols / 128) panels of 128 and the Gram np (np + 1) / 2 panel pairs (I <= J).
// A block of 4 waves takes ONE pair and a fixed, contiguous row range (a function of rows and np alone),
// stages 32 rows of its panel(s) at a time in LDS and accumulates
//   * a diagonal pair (I == J): the 36 upper-triangle 16x16 tiles, 9 per wave, and the panel's column sums;
//   * an off-diagonal pair: all 64 tiles, wave w the tile rows 2w, 2w + 1 (16 tiles, 10 LDS reads per
//     16 MFMAs).
// Blocks of one row range are neighbours in the grid (block = range * pairs + pair), so the panels that the
// pairs share are re-read from the cache.  Each block writes its partial tiles to its slot of the workspace;
// a finish kernel adds the slots of a pair in range order and mirrors the tiles.  No atomics: the result
// depends on (rows, cols) only.
#include "p2l_common.h"

namespace {

constexpr int kThreads = 256;            // 4 waves
constexpr int kRows = 32;                // rows per LDS chunk
constexpr int kPanel = 128;              // columns per panel
constexpr int kMaxCols = 512;
constexpr int kPerThread = kRows * kPanel / kThreads;
constexpr int kLds = 144;                // LDS row stride (floats): the 4 rows of a fragment on disjoint banks
constexpr int kDiagTiles = 36;           // upper-triangle 16x16 tiles of 128 x 128
constexpr int kOffTiles = 64;
constexpr int kSlotDoubles = kOffTiles * 256 + kPanel;   // one block's partial: tiles, then column sums
constexpr int kMaxBlocks = 512;          // 2 blocks per CU
constexpr int kMinChunksPerBlock = 8;    // a block writes 128 KB of partials: at least 256 rows behind them
constexpr int kFinishThreads = 64;

typedef double d4 __attribute__((ext_vector_type(4)));

// tile p of the upper triangle of a diagonal pair in row-major order: (ti, tj) with ti <= tj
__constant__ unsigned char kPairs[kDiagTiles][2] = {
    {0, 0}, {0, 1}, {0, 2}, {0, 3}, {0, 4}, {0, 5}, {0, 6}, {0, 7}, {1, 1}, {1, 2}, {1, 3}, {1, 4},
    {1, 5}, {1, 6}, {1, 7}, {2, 2}, {2, 3}, {2, 4}, {2, 5}, {2, 6}, {2, 7}, {3, 3}, {3, 4}, {3, 5},
    {3, 6}, {3, 7}, {4, 4}, {4, 5}, {4, 6}, {4, 7}, {5, 5}, {5, 6}, {5, 7}, {6, 6}, {6, 7}, {7, 7}};

struct WidePlan {
  int npan, npairs;
  int nrange;           // row ranges (blocks = nrange * npairs = slots in the workspace)
  int64_t range_rows;   // rows per range, a multiple of kRows (the last range may own fewer)
};

WidePlan wide_plan(int64_t rows, int cols) {
  WidePlan p;
  p.npan = (cols + kPanel - 1) / kPanel;
  p.npairs = p.npan * (p.npan + 1) / 2;
  const int64_t nchunks = (rows + kRows - 1) / kRows;
  int64_t nr = (nchunks + kMinChunksPerBlock - 1) / kMinChunksPerBlock;
  if (nr > kMaxBlocks / p.npairs) nr = kMaxBlocks / p.npairs;
  const int64_t cpr = (nchunks + nr - 1) / nr;
  p.nrange = (int)((nchunks + cpr - 1) / cpr);         // no range without rows
  p.range_rows = cpr * kRows;
  return p;
}

bool wide_args_ok(int64_t rows, int cols, int64_t ld) {
  return rows >= 1 && cols >= 1 && cols <= kMaxCols && ld >= cols;
}

// pair p of np panels in row-major order of the upper triangle: (I, J) with I <= J
__device__ __forceinline__ void pair_of(int p, int np, int& I, int& J) {
  I = 0;
  while (p >= np - I) {
    p -= np - I;
    ++I;
  }
  J = I + p;
}

// kRows rows of the panel that starts at column c0, from row r0 on; zero outside the panel and the block's rows
__device__ __forceinline__ void load_chunk(const float* __restrict__ X, int64_t r0, int64_t r_end, int c0, int cols,
                                           int64_t ld, int tid, float (&v)[kPerThread]) {
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int idx = tid + k * kThreads;
    const int64_t gr = r0 + (idx >> 7);
    const int gc = c0 + (idx & 127);
    float x = 0.0f;
    if (gr < r_end && gc < cols) x = X[gr * ld + gc];
    v[k] = x;
  }
}

__device__ __forceinline__ void store_chunk(float (*s)[kLds], int tid, const float (&v)[kPerThread]) {
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int idx = tid + k * kThreads;
    s[idx >> 7][idx & 127] = v[k];
  }
}

// one panel pair over the rows [r_begin, r_end): panel I starts at column cI, panel J at cJ
template <bool DIAG>
__device__ __forceinline__ void gram_pair(const float* __restrict__ X, int64_t r_begin, int64_t r_end, int cols,
                                          int64_t ld, int cI, int cJ, float (*sI)[kLds], float (*sJ)[kLds],
                                          double* __restrict__ out) {
  constexpr int kAcc = DIAG ? kDiagTiles / 4 : kOffTiles / 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int left = (cols - cJ + 15) >> 4;
  const int ntJ = left < 8 ? left : 8;               // 16-column tiles of panel J that hold columns

  d4 acc[kAcc];
#pragma unroll
  for (int q = 0; q < kAcc; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
  double csum = 0.0;

  float vI[kPerThread], vJ[kPerThread];
  load_chunk(X, r_begin, r_end, cI, cols, ld, tid, vI);
  if (!DIAG) load_chunk(X, r_begin, r_end, cJ, cols, ld, tid, vJ);
  for (int64_t r0 = r_begin; r0 < r_end; r0 += kRows) {
    store_chunk(sI, tid, vI);
    if (!DIAG) store_chunk(sJ, tid, vJ);
    __syncthreads();
    if (r0 + kRows < r_end) {                        // in flight meanwhile
      load_chunk(X, r0 + kRows, r_end, cI, cols, ld, tid, vI);
      if (!DIAG) load_chunk(X, r0 + kRows, r_end, cJ, cols, ld, tid, vJ);
    }

    if (DIAG && tid < kPanel) {
#pragma unroll 8
      for (int r = 0; r < kRows; ++r) csum += (double)sI[r][tid];
    }
    // tile (ti, tj) += A B with A[i][k] = X[row k][cI + 16 ti + i], B[k][j] = X[row k][cJ + 16 tj + j]:
    // lane l holds k = l >> 4 and i = j = l & 15
    // (4 of the 8 steps unrolled: 122 + 128 accumulator registers, two waves per SIMD; all 8 take 158 + 128, one)
#pragma unroll 4
    for (int st = 0; st < kRows / 4; ++st) {
      const float* rowI = &sI[4 * st + (lane >> 4)][lane & 15];
      if (DIAG) {
#pragma unroll
        for (int q = 0; q < kAcc; ++q) {
          const int p = wave + 4 * q;
          const int ti = kPairs[p][0], tj = kPairs[p][1];
          if (tj < ntJ) {
            const double a = (double)rowI[16 * ti], b = (double)rowI[16 * tj];
            acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
          }
        }
      } else {
        const float* rowJ = &sJ[4 * st + (lane >> 4)][lane & 15];
        const double a0 = (double)rowI[32 * wave], a1 = (double)rowI[32 * wave + 16];
#pragma unroll
        for (int tj = 0; tj < 8; ++tj) {
          if (tj < ntJ) {
            const double b = (double)rowJ[16 * tj];
            acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[tj], 0, 0, 0);
            acc[8 + tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[8 + tj], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  // C/D of the f64 form: column lane & 15, row (lane >> 4) + 4 * reg (not the f32 forms' map)
#pragma unroll
  for (int q = 0; q < kAcc; ++q) {
    // diagonal: tile p of kPairs; off-diagonal: tile ti * 8 + tj with ti = 2 wave + (q >> 3), tj = q & 7
    const int t = DIAG ? wave + 4 * q : (2 * wave + (q >> 3)) * 8 + (q & 7);
    if (!DIAG && (q & 7) >= ntJ) continue;           // never accumulated, never read by the finish kernel
#pragma unroll
    for (int g = 0; g < 4; ++g) out[t * 256 + ((lane >> 4) + 4 * g) * 16 + (lane & 15)] = acc[q][g];
  }
  if (DIAG && tid < kPanel) out[kOffTiles * 256 + tid] = csum;
}

__global__ __launch_bounds__(kThreads) void gram_wide_kernel(const float* __restrict__ X, int64_t rows, int cols,
                                                             int64_t ld, int npan, int npairs, int64_t range_rows,
                                                             double* __restrict__ part) {
  __shared__ float s[2][kRows][kLds];
  const int range = blockIdx.x / npairs, pair = blockIdx.x - range * npairs;
  int I, J;
  pair_of(pair, npan, I, J);
  const int64_t r_begin = (int64_t)range * range_rows;
  const int64_t r_end = r_begin + range_rows < rows ? r_begin + range_rows : rows;
  double* out = part + (size_t)blockIdx.x * kSlotDoubles;
  if (I == J)
    gram_pair<true>(X, r_begin, r_end, cols, ld, I * kPanel, J * kPanel, s[0], s[0], out);
  else
    gram_pair<false>(X, r_begin, r_end, cols, ld, I * kPanel, J * kPanel, s[0], s[1], out);
}

// entry e of a pair's slots (kOffTiles x 256 tile entries, then 128 column sums), summed in range order
__global__ __launch_bounds__(kFinishThreads) void gram_wide_finish_kernel(const double* __restrict__ part, int nrange,
                                                                          int npan, int npairs, int cols,
                                                                          double* __restrict__ gram,
                                                                          double* __restrict__ colsum) {
  const int e = blockIdx.x * kFinishThreads + threadIdx.x;
  const int pair = blockIdx.y;
  if (e >= kSlotDoubles) return;
  int I, J;
  pair_of(pair, npan, I, J);
  int i = 0, j;
  bool tile = e < kOffTiles * 256;
  if (tile) {
    const int t = e >> 8, a = (e >> 4) & 15, c = e & 15;
    int ti, tj;
    if (I == J) {
      if (t >= kDiagTiles) return;
      ti = kPairs[t][0], tj = kPairs[t][1];
      if (ti == tj && a > c) return;                 // a diagonal tile: its upper half, mirrored
    } else {
      ti = t >> 3, tj = t & 7;
    }
    i = I * kPanel + 16 * ti + a, j = J * kPanel + 16 * tj + c;
    if (i >= cols || j >= cols) return;
  } else {
    if (I != J) return;                              // the column sums come from the diagonal pairs
    j = I * kPanel + (e - kOffTiles * 256);
    if (j >= cols) return;
  }
  double t = 0.0;
  // (the adds stay one chain in range order; unrolling only puts 16 loads in flight instead of one)
#pragma unroll 16
  for (int r = 0; r < nrange; ++r) t += part[((size_t)r * npairs + pair) * kSlotDoubles + e];
  if (!tile) {
    colsum[j] = t;
    return;
  }
  gram[(size_t)i * cols + j] = t;
  gram[(size_t)j * cols + i] = t;
}

}  // namespace

extern "C" size_t p2l_gram_f64_wide_ws_bytes(int64_t rows, int cols) {
  if (!wide_args_ok(rows, cols, cols)) return 0;
  const WidePlan p = wide_plan(rows, cols);
  return (size_t)p.nrange * p.npairs * kSlotDoubles * sizeof(double);
}

extern "C" int p2l_gram_f64_wide(const float* X, int64_t rows, int cols, int64_t ld, double* gram, double* colsum,
                                 void* ws, size_t ws_bytes, void* stream) {
  if (!X || !gram || !colsum || !wide_args_ok(rows, cols, ld)) return P2L_EINVAL;
  const size_t need = p2l_gram_f64_wide_ws_bytes(rows, cols);
  if (!ws || ws_bytes < need) return P2L_EWS;
  hipStream_t st = (hipStream_t)stream;
  const WidePlan p = wide_plan(rows, cols);
  double* part = (double*)ws;
  hipLaunchKernelGGL(gram_wide_kernel, dim3(p.nrange * p.npairs), dim3(kThreads), 0, st, X, rows, cols, ld, p.npan,
                     p.npairs, p.range_rows, part);
  hipLaunchKernelGGL(gram_wide_finish_kernel, dim3(cdiv(kSlotDoubles, kFinishThreads), p.npairs),
                     dim3(kFinishThreads), 0, st, part, p.nrange, p.npan, p.npairs, cols, gram, colsum);
  return p2l_check_launch();
}
