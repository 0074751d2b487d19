// fp64 Gram of a tall fp32 panel: G = X^T X ([cols][cols]) and the column sums of X, the only
// O(rows) work of the GANSpace components (pix2latent_amd/edit/ganspace.py).
//
// X has `rows` rows and 1 <= cols <= 128 columns, element (r, j) at X[r * ld + j] (trans = 0) or
// X[j * ld + r] (trans = 1: the z-rows of the packed gen_z weight).  Products of fp32 operands are
// exact in fp64; v_mfma_f64_16x16x4_f64 sums them.
//
// The 128 columns form 8 tiles of 16; only the 36 tiles (ti <= tj) of the upper triangle are
// computed.  A block of 4 waves owns a fixed, contiguous row range (a function of `rows` alone),
// stages it 32 rows at a time in LDS, and each wave accumulates 9 of the 36 tiles; the block writes
// its partial tiles and column sums to the workspace.  A finish kernel adds the partials of all
// blocks in block order and mirrors the tiles.  No atomics: the result depends on (rows, cols, trans)
// only.
#include "p2l_common.h"

namespace {

constexpr int kThreads = 256;            // 4 waves
constexpr int kRows = 32;                // rows per LDS chunk
constexpr int kPerThread = kRows * 128 / kThreads;
constexpr int kLds = 144;                // LDS row stride (floats): the 4 rows of a fragment on disjoint banks
constexpr int kTiles = 36;               // upper-triangle 16x16 tiles of 128 x 128
constexpr int kPartDoubles = kTiles * 256 + 128;      // one block's partial: tiles, then column sums
constexpr int kMaxBlocks = 512;          // 2 blocks per CU
constexpr int kMinChunksPerBlock = 4;
constexpr int kFinishThreads = 64;

typedef double d4 __attribute__((ext_vector_type(4)));

// tile p of the upper triangle in row-major order: (ti, tj) with ti <= tj
__constant__ unsigned char kPairs[kTiles][2] = {
    {0, 0}, {0, 1}, {0, 2}, {0, 3}, {0, 4}, {0, 5}, {0, 6}, {0, 7}, {1, 1}, {1, 2}, {1, 3}, {1, 4},
    {1, 5}, {1, 6}, {1, 7}, {2, 2}, {2, 3}, {2, 4}, {2, 5}, {2, 6}, {2, 7}, {3, 3}, {3, 4}, {3, 5},
    {3, 6}, {3, 7}, {4, 4}, {4, 5}, {4, 6}, {4, 7}, {5, 5}, {5, 6}, {5, 7}, {6, 6}, {6, 7}, {7, 7}};

struct GramPlan {
  int nblk;             // blocks (= partials in the workspace)
  int64_t blk_rows;     // rows per block, a multiple of kRows (the last block may own fewer)
};

GramPlan gram_plan(int64_t rows) {
  const int64_t nchunks = (rows + kRows - 1) / kRows;
  int64_t nblk = (nchunks + kMinChunksPerBlock - 1) / kMinChunksPerBlock;
  if (nblk > kMaxBlocks) nblk = kMaxBlocks;
  const int64_t cpb = (nchunks + nblk - 1) / nblk;
  GramPlan p;
  p.nblk = (int)((nchunks + cpb - 1) / cpb);           // no block without rows
  p.blk_rows = cpb * kRows;
  return p;
}

bool gram_args_ok(int64_t rows, int cols, int64_t ld, int trans) {
  if (rows < 1 || cols < 1 || cols > 128 || (trans != 0 && trans != 1)) return false;
  return trans == 0 ? ld >= cols : ld >= rows;
}

// element k of a thread's share of a chunk: row r, column j
template <int TRANS>
__device__ __forceinline__ void chunk_pos(int tid, int k, int& r, int& j) {
  const int idx = tid + k * kThreads;
  r = TRANS ? (idx & (kRows - 1)) : (idx >> 7);
  j = TRANS ? (idx / kRows) : (idx & 127);
}

// kRows rows x 128 columns from row r0 on, zero outside the panel and the block's rows
template <int TRANS>
__device__ __forceinline__ void load_chunk(const float* __restrict__ X, int64_t r0, int64_t r_end, int cols,
                                           int64_t ld, int tid, float (&v)[kPerThread]) {
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    int r, j;
    chunk_pos<TRANS>(tid, k, r, j);
    const int64_t gr = r0 + r;
    float x = 0.0f;
    if (gr < r_end && j < cols) x = TRANS ? X[(int64_t)j * ld + gr] : X[gr * ld + j];
    v[k] = x;
  }
}

template <int TRANS>
__global__ __launch_bounds__(kThreads) void gram_f64_kernel(const float* __restrict__ X, int64_t rows, int cols,
                                                            int64_t ld, int64_t blk_rows, double* __restrict__ part) {
  __shared__ float s[kRows][kLds];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = (cols + 15) >> 4;
  const int64_t r_begin = (int64_t)blockIdx.x * blk_rows;
  const int64_t r_end = r_begin + blk_rows < rows ? r_begin + blk_rows : rows;

  d4 acc[kTiles / 4];
#pragma unroll
  for (int q = 0; q < kTiles / 4; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
  double csum = 0.0;

  float v[kPerThread];
  load_chunk<TRANS>(X, r_begin, r_end, cols, ld, tid, v);
  for (int64_t r0 = r_begin; r0 < r_end; r0 += kRows) {
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      int r, j;
      chunk_pos<TRANS>(tid, k, r, j);
      s[r][j] = v[k];
    }
    __syncthreads();
    if (r0 + kRows < r_end) load_chunk<TRANS>(X, r0 + kRows, r_end, cols, ld, tid, v);   // in flight meanwhile

    if (tid < 128) {
#pragma unroll 8
      for (int r = 0; r < kRows; ++r) csum += (double)s[r][tid];
    }
    // tile (ti, tj) += A B with A[i][k] = X[row k][16 ti + i], B[k][j] = X[row k][16 tj + j]:
    // lane l holds k = l >> 4 and i = j = l & 15
#pragma unroll
    for (int st = 0; st < kRows / 4; ++st) {
      const float* row = &s[4 * st + (lane >> 4)][lane & 15];
#pragma unroll
      for (int q = 0; q < kTiles / 4; ++q) {
        const int p = wave + 4 * q;
        const int ti = kPairs[p][0], tj = kPairs[p][1];
        if (tj < nt) {
          const double a = (double)row[16 * ti], b = (double)row[16 * tj];
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // C/D of the f64 form: column lane & 15, row (lane >> 4) + 4 * reg (not the f32 forms' map)
  double* out = part + (size_t)blockIdx.x * kPartDoubles;
#pragma unroll
  for (int q = 0; q < kTiles / 4; ++q) {
    const int p = wave + 4 * q;
#pragma unroll
    for (int g = 0; g < 4; ++g) out[p * 256 + ((lane >> 4) + 4 * g) * 16 + (lane & 15)] = acc[q][g];
  }
  if (tid < 128) out[kTiles * 256 + tid] = csum;
}

// entry e of the partials (kTiles x 256 tile entries, then 128 column sums), summed in block order
__global__ __launch_bounds__(kFinishThreads) void gram_f64_finish_kernel(const double* __restrict__ part, int nblk,
                                                                         int cols, double* __restrict__ gram,
                                                                         double* __restrict__ colsum) {
  const int e = blockIdx.x * kFinishThreads + threadIdx.x;
  if (e >= kPartDoubles) return;
  double t = 0.0;
  // (the adds stay one chain in block order; unrolling only puts 16 loads in flight instead of one)
#pragma unroll 16
  for (int b = 0; b < nblk; ++b) t += part[(size_t)b * kPartDoubles + e];
  if (e >= kTiles * 256) {
    const int j = e - kTiles * 256;
    if (j < cols) colsum[j] = t;
    return;
  }
  const int p = e >> 8, a = (e >> 4) & 15, c = e & 15;
  const int ti = kPairs[p][0], tj = kPairs[p][1];
  if (ti == tj && a > c) return;                   // a diagonal tile: its upper half, mirrored
  const int i = 16 * ti + a, j = 16 * tj + c;
  if (i >= cols || j >= cols) return;
  gram[(size_t)i * cols + j] = t;
  gram[(size_t)j * cols + i] = t;
}

}  // namespace

extern "C" size_t p2l_gram_f64_ws_bytes(int64_t rows, int cols, int trans) {
  if (!gram_args_ok(rows, cols, trans == 0 ? cols : rows, trans)) return 0;
  return (size_t)gram_plan(rows).nblk * kPartDoubles * sizeof(double);
}

extern "C" int p2l_gram_f64(const float* X, int64_t rows, int cols, int64_t ld, int trans, double* gram,
                            double* colsum, void* ws, size_t ws_bytes, void* stream) {
  if (!X || !gram || !colsum || !gram_args_ok(rows, cols, ld, trans)) return P2L_EINVAL;
  const size_t need = p2l_gram_f64_ws_bytes(rows, cols, trans);
  if (!ws || ws_bytes < need) return P2L_EWS;
  hipStream_t st = (hipStream_t)stream;
  const GramPlan p = gram_plan(rows);
  double* part = (double*)ws;
  if (trans)
    hipLaunchKernelGGL(gram_f64_kernel<1>, dim3(p.nblk), dim3(kThreads), 0, st, X, rows, cols, ld, p.blk_rows, part);
  else
    hipLaunchKernelGGL(gram_f64_kernel<0>, dim3(p.nblk), dim3(kThreads), 0, st, X, rows, cols, ld, p.blk_rows, part);
  hipLaunchKernelGGL(gram_f64_finish_kernel, dim3(cdiv(kPartDoubles, kFinishThreads)), dim3(kFinishThreads), 0, st,
                     part, p.nblk, cols, gram, colsum);
  return p2l_check_launch();
}
