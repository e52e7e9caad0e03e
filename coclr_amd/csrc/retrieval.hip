// Evaluation consumers of the backbone for gfx950:
//   * LinearClassifier head (model/classifier.py:47-61): BatchNorm1d statistics of the pooled
//     (N, C) features (final_bn) -- the rest of the head reuses the GEMM / l2norm / BN kernels
//   * nearest-neighbour retrieval (eval/main_classifier.py:686-706): centre and normalise the
//     feature matrices, sim = test . train^T, then for k in (1,5,10,20,50) "is any of the k most
//     similar training clips of the test clip's class": one kernel selects the top-kmax of every
//     similarity row IN ORDER and compares labels on the way, instead of five torch.topk calls
//     over the full (n_test, n_train) matrix
//   * video-level scores of the test modes (eval/main_classifier.py:488,533,637,673): clips of one video are
//     rows of a fixed-size batch; per video, out += weight * sum over its rows of softmax(row) (or of the row
//     itself, for features) -- a segmented accumulate, because a batch cuts across video boundaries
//   * two-stream test fusion (eval/merge_2stream_prob.py:80-98): the float64 mean of two probability rows and
//     the first maximum of either row and of the mean, one wave per video
#include "common.h"
#include "../../include/coclr_hip.h"
#include <math.h>

namespace {

// partial[r][c] = sum over rows r, r+R, ... of x[row][c]  (and of x^2 when `sq`)
__global__ void __launch_bounds__(256)
colsum_partial_kernel(const float* __restrict__ x, float* __restrict__ part,
                      float* __restrict__ part_sq, int rows, int cols) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const int R = gridDim.y, r0 = blockIdx.y;
  float s = 0.f, q = 0.f;
  for (int r = r0; r < rows; r += R) {
    const float v = x[(long)r * cols + c];
    s += v;
    q = fmaf(v, v, q);
  }
  part[(long)r0 * cols + c] = s;
  if (part_sq) part_sq[(long)r0 * cols + c] = q;
}

// out[r][c] = x[r][c] - mean[c], mean from the R partial sums (fp64 fold)
__global__ void __launch_bounds__(256)
center_rows_kernel(const float* __restrict__ x, const float* __restrict__ part, float* __restrict__ out,
                   int rows, int cols, int R) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0;
  for (int r = 0; r < R; ++r) s += part[(long)r * cols + c];
  const float mean = (float)(s / rows);
  for (int r = blockIdx.y; r < rows; r += gridDim.y)
    out[(long)r * cols + c] = x[(long)r * cols + c] - mean;
}

// stats[0][c] = sum_r x[r][c], stats[1][c] = sum_r x[r][c]^2   (one "tile" per channel: the
// layout coclr_bn_finalize takes with ntiles = 1)
__global__ void __launch_bounds__(256)
bn1d_fold_kernel(const float* __restrict__ part, const float* __restrict__ part_sq,
                 float* __restrict__ stats, int cols, int R) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0, q = 0.0;
  for (int r = 0; r < R; ++r) { s += part[(long)r * cols + c]; q += part_sq[(long)r * cols + c]; }
  stats[c] = (float)s;
  stats[cols + c] = (float)q;
}

// Ordered top-kmax of one similarity row; hits[b][i] = any(train_label[top ks[i]] == test_label[b]).
// Selection order is (value descending, column ascending); the t-th pick is the largest element
// that comes strictly after the (t-1)-th in that order, so nothing is marked or modified.
__global__ void __launch_bounds__(256)
retrieval_hits_kernel(const float* __restrict__ sim, const int64_t* __restrict__ train_label,
                      const int64_t* __restrict__ test_label, const int32_t* __restrict__ ks, int nk,
                      int kmax, float* __restrict__ hits, int32_t* __restrict__ topidx, int N,
                      int use_lds) {
  extern __shared__ float rowbuf[];
  __shared__ float wbest[4];
  __shared__ int widx[4];
  __shared__ float s_pv;
  __shared__ int s_pi;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = sim + (long)b * N;
  if (use_lds) {
    for (int j = tid; j < N; j += 256) rowbuf[j] = row[j];
  }
  const int64_t want = test_label[b];
  if (tid == 0) { s_pv = INFINITY; s_pi = -1; }
  bool found = false;      // thread 0 only
  int next_k = 0;
  __syncthreads();
  for (int t = 0; t < kmax; ++t) {
    const float pv = s_pv;
    const int pi = s_pi;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = tid; j < N; j += 256) {
      const float v = use_lds ? rowbuf[j] : row[j];
      const bool eligible = (v < pv) || (v == pv && j > pi);
      if (eligible && (v > best || (v == best && j < bi))) { best = v; bi = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(bi, off);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) {
        best = ob; bi = oi;
      }
    }
    if ((tid & 63) == 0) { wbest[tid >> 6] = best; widx[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        if (widx[w] != 0x7fffffff &&
            (bi == 0x7fffffff || wbest[w] > best || (wbest[w] == best && widx[w] < bi))) {
          best = wbest[w]; bi = widx[w];
        }
      if (bi != 0x7fffffff) {
        if (train_label[bi] == want) found = true;
        if (topidx) topidx[(long)b * kmax + t] = bi;
        s_pv = best; s_pi = bi;
      } else if (topidx) {
        topidx[(long)b * kmax + t] = -1;
      }
      while (next_k < nk && ks[next_k] == t + 1) { hits[(long)b * nk + next_k] = found ? 1.f : 0.f; ++next_k; }
    }
    __syncthreads();
  }
}

// ---- two-stream score fusion ----------------------------------------------------------------------------
// (value descending, column ascending): the order of retrieval_hits_kernel, on doubles.  A slot that has seen
// no column carries FUSE_NONE and loses to any column.
#define FUSE_NONE 0x7fffffff
__device__ __forceinline__ void fuse_take(double& best, int& bi, double v, int c) {
  if (c != FUSE_NONE && (bi == FUSE_NONE || v > best || (v == best && c < bi))) { best = v; bi = c; }
}

// One wave per video, four videos per workgroup; lanes stride over the C columns.  fused[v][c] = (p1 + p2) * 0.5
// in double (what numpy forms from the two fp32 rows, merge_2stream_prob.py:95), and the first maximum of p1, p2
// and the mean (np.argmax, :96-98) as argmax[v][0..2]; hits[v][i] = argmax[v][i] == label[v].
__global__ void __launch_bounds__(256)
fuse_scores_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                   const int64_t* __restrict__ label, double* __restrict__ fused,
                   int32_t* __restrict__ argmax, float* __restrict__ hits, int V, int C) {
  const int lane = threadIdx.x & 63;
  const long v = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= V) return;                           // whole waves leave: the shuffles below see 64 lanes
  const float* a = p1 + v * C;
  const float* b = p2 + v * C;
  double* o = fused + v * C;
  double best[3] = {0.0, 0.0, 0.0};
  int bi[3] = {FUSE_NONE, FUSE_NONE, FUSE_NONE};
  for (int c = lane; c < C; c += 64) {
    const double x = (double)a[c], y = (double)b[c];
    const double f = (x + y) * 0.5;
    o[c] = f;
    fuse_take(best[0], bi[0], x, c);
    fuse_take(best[1], bi[1], y, c);
    fuse_take(best[2], bi[2], f, c);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double ob = __shfl_xor(best[j], off);
      const int oi = __shfl_xor(bi[j], off);
      fuse_take(best[j], bi[j], ob, oi);
    }
  }
  if (lane == 0) {                              // lane 0 owns column 0: bi is a column of the row
    const int64_t want = label[v];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      argmax[v * 3 + j] = bi[j];
      hits[v * 3 + j] = (int64_t)bi[j] == want ? 1.f : 0.f;
    }
  }
}

// ---- segmented accumulate -------------------------------------------------------------------------------
// The segments of one launch travel by value in the kernel arguments (1 KB): the host validates them and
// nothing is copied to the device.  No two segments of one launch write the same output row.
#define COCLR_SEG_MAX 64
#define COCLR_SEG_MAX_C 4096
struct SegBatch {
  int first[COCLR_SEG_MAX];
  int rows[COCLR_SEG_MAX];
  int out[COCLR_SEG_MAX];
  float w[COCLR_SEG_MAX];
};

template <int VEC> struct SegVec;
template <> struct SegVec<1> { using T = float; };
template <> struct SegVec<4> { using T = f32x4; };

__device__ __forceinline__ float seg_hmax(float v) { return v; }
__device__ __forceinline__ float seg_hmax(f32x4 v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
__device__ __forceinline__ float seg_hsum(float v) { return v; }
__device__ __forceinline__ float seg_hsum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float seg_exp(float v, float m) { return expf(v - m); }
__device__ __forceinline__ f32x4 seg_exp(f32x4 v, float m) {
  f32x4 e;
  e.x = expf(v.x - m); e.y = expf(v.y - m); e.z = expf(v.z - m); e.w = expf(v.w - m);
  return e;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// One workgroup per segment: out[o][:] += w * sum_{r ascending} f(x[first + r][:]), f = softmax or identity.
// A thread owns the columns (tid + 256 k) * VEC .. + VEC of every row, so the per-column sums are formed by
// one thread in row order (fp32): the result does not depend on scheduling.  VEC = 4: 16-byte loads and stores
// (C % 4 == 0, 16-byte aligned bases).  Softmax keeps the running sums and the row in LDS (2 * C floats).
template <int VEC, bool SOFTMAX>
__global__ void __launch_bounds__(256)
segment_accum_kernel(const float* __restrict__ x, float* __restrict__ out, int C, SegBatch sb) {
  using T = typename SegVec<VEC>::T;
  extern __shared__ __attribute__((aligned(16))) float seg_lds[];
  __shared__ float red_max[4], red_sum[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int first = sb.first[s], rows = sb.rows[s];
  const float wgt = sb.w[s];
  const int CV = C / VEC;                       // columns in units of T
  T* o = reinterpret_cast<T*>(out + (long)sb.out[s] * C);
  if (!SOFTMAX) {
    for (int c = tid; c < CV; c += 256) {
      T acc = T(0.f);
      for (int r = 0; r < rows; ++r)
        acc += reinterpret_cast<const T*>(x + (long)(first + r) * C)[c];
      o[c] += wgt * acc;
    }
    return;
  }
  T* acc = reinterpret_cast<T*>(seg_lds);
  T* row = reinterpret_cast<T*>(seg_lds + C);
  for (int c = tid; c < CV; c += 256) acc[c] = T(0.f);
  for (int r = 0; r < rows; ++r) {
    const T* xr = reinterpret_cast<const T*>(x + (long)(first + r) * C);
    float m = -INFINITY;
    for (int c = tid; c < CV; c += 256) {
      const T v = xr[c];
      row[c] = v;
      m = fmaxf(m, seg_hmax(v));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) red_max[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));
    float sum = 0.f;
    for (int c = tid; c < CV; c += 256) {
      const T e = seg_exp(row[c], m);
      row[c] = e;
      sum += seg_hsum(e);
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red_sum[tid >> 6] = sum;
    __syncthreads();
    sum = (red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]);
    for (int c = tid; c < CV; c += 256) acc[c] += row[c] / sum;
  }
  for (int c = tid; c < CV; c += 256) o[c] += wgt * acc[c];
}

}  // namespace

extern "C" int coclr_colstats_workspace(int rows, int cols, int64_t* elems) {
  if (rows <= 0 || cols <= 0) return COCLR_EINVAL;
  int R = rows < 64 ? rows : 64;
  *elems = (int64_t)2 * R * cols;
  return 0;
}

static int row_splits(int rows) { return rows < 64 ? rows : 64; }

// BatchNorm1d batch statistics of x[rows][cols] as [2][cols] (= coclr_bn_finalize, ntiles 1)
extern "C" int coclr_bn1d_stats(const float* x, float* stats, float* workspace, int rows, int cols,
                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (rows <= 0 || cols <= 0 || !x || !stats || !workspace) return COCLR_EINVAL;
  const int R = row_splits(rows);
  float* part = workspace;
  float* part_sq = workspace + (long)R * cols;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(cdiv(cols, 256), R), dim3(256), 0, stream, x, part,
                     part_sq, rows, cols);
  COCLR_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn1d_fold_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, stream, part, part_sq,
                     stats, cols, R);
  COCLR_LAUNCH_CHECK();
  return 0;
}

// out = x - x.mean(0)   (eval/main_classifier.py:690-691)
extern "C" int coclr_center_rows(const float* x, float* out, float* workspace, int rows, int cols,
                                 void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (rows <= 0 || cols <= 0 || !x || !out || !workspace) return COCLR_EINVAL;
  const int R = row_splits(rows);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(cdiv(cols, 256), R), dim3(256), 0, stream, x,
                     workspace, (float*)nullptr, rows, cols);
  COCLR_LAUNCH_CHECK();
  int gy = rows < 256 ? rows : 256;
  hipLaunchKernelGGL(center_rows_kernel, dim3(cdiv(cols, 256), gy), dim3(256), 0, stream, x,
                     workspace, out, rows, cols, R);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_retrieval_hits(const float* sim, const int64_t* train_label,
                                    const int64_t* test_label, const int32_t* ks, int nk,
                                    float* hits, int32_t* topidx, int B, int N, int kmax,
                                    void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || N <= 0 || nk <= 0 || kmax <= 0 || kmax > N || !sim || !ks || !hits) return COCLR_EINVAL;
  auto kern = retrieval_hits_kernel;
  const size_t lds_row = (size_t)N * sizeof(float);
  const int use_lds = lds_row <= 150 * 1024;
  static std::atomic<uint64_t> attr_done{0};
  COCLR_RETURN_IF(ensure_dyn_lds(reinterpret_cast<const void*>(kern), 150 * 1024, attr_done));
  hipLaunchKernelGGL(kern, dim3(B), dim3(256), use_lds ? lds_row : 0, stream, sim, train_label,
                     test_label, ks, nk, kmax, hits, topidx, N, use_lds);
  COCLR_LAUNCH_CHECK();
  return 0;
}

// (p1 + p2) / 2 and the three arg-maxima of eval/merge_2stream_prob.py:80-98
extern "C" int coclr_fuse_scores(const float* p1, const float* p2, const int64_t* label, double* fused,
                                 int32_t* argmax, float* hits, int V, int C, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (V <= 0 || C <= 0 || !p1 || !p2 || !label || !fused || !argmax || !hits) return COCLR_EINVAL;
  hipLaunchKernelGGL(fuse_scores_kernel, dim3(cdiv(V, 4)), dim3(256), 0, stream, p1, p2, label, fused,
                     argmax, hits, V, C);
  COCLR_LAUNCH_CHECK();
  return 0;
}

template <bool SOFTMAX>
static int segment_accum(const float* x, const int32_t* segs, const float* weight, float* out, int R, int C,
                         int S, int V, hipStream_t stream) {
  if (!x || !segs || !weight || !out || R <= 0 || S <= 0 || V <= 0 || C < 1 || C > COCLR_SEG_MAX_C)
    return COCLR_EINVAL;
  for (int s = 0; s < S; ++s) {                 // everything is checked before anything is launched
    const long first = segs[3 * s], rows = segs[3 * s + 1], o = segs[3 * s + 2];
    if (first < 0 || rows < 1 || first + rows > R || o < 0 || o >= V) return COCLR_EINVAL;
  }
  const bool vec = C % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  const size_t lds = SOFTMAX ? (size_t)2 * C * sizeof(float) : 0;
  SegBatch sb;
  int n = 0;
  for (int s = 0; s <= S; ++s) {
    bool flush = s == S || n == COCLR_SEG_MAX;
    // a second segment of the same output row (another crop of the video in this batch) goes into the
    // next launch: the stream orders the two read-modify-writes
    for (int j = 0; j < n && !flush; ++j) flush = sb.out[j] == segs[3 * s + 2];
    if (flush && n > 0) {
      if (vec)
        hipLaunchKernelGGL((segment_accum_kernel<4, SOFTMAX>), dim3(n), dim3(256), lds, stream, x, out, C, sb);
      else
        hipLaunchKernelGGL((segment_accum_kernel<1, SOFTMAX>), dim3(n), dim3(256), lds, stream, x, out, C, sb);
      COCLR_LAUNCH_CHECK();
      n = 0;
    }
    if (s == S) break;
    sb.first[n] = segs[3 * s]; sb.rows[n] = segs[3 * s + 1]; sb.out[n] = segs[3 * s + 2];
    sb.w[n] = weight[s];
    ++n;
  }
  return 0;
}

extern "C" int coclr_segment_softmax_accum(const float* logits, const int32_t* segs, const float* weight,
                                           float* out, int R, int C, int S, int V, void* stream) {
  return segment_accum<true>(logits, segs, weight, out, R, C, S, V, (hipStream_t)stream);
}

extern "C" int coclr_segment_accum(const float* x, const int32_t* segs, const float* weight, float* out,
                                   int R, int C, int S, int V, void* stream) {
  return segment_accum<false>(x, segs, weight, out, R, C, S, V, (hipStream_t)stream);
}
