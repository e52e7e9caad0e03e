// Loss + accuracy epilogue over the (B, 1+K) logits for gfx950 -- what the launch scripts compute
// with 8-12 ATen ops and 3-5 .item() syncs per step:
//   InfoNCE  main_nce.py:314-316   CrossEntropyLoss(output, target) + calc_topk_accuracy(1,5)
//   UberNCE  main_nce.py:318-324   -(log_softmax*mask).sum(1)/mask.sum(1), calc_mask_accuracy(1,5)
//   CoCLR    main_coclr.py:343-346,388-401  multi_nce_loss = -log((softmax*mask).sum(1)) with the
//            self-similarity column dropped for rows that have other positives, calc_mask_accuracy
//            and calc_topk_accuracy against column 0   (utils/utils.py:52-85)
// One workgroup per row reads the row twice (max, then exp-sums / counts; the second pass hits
// L2), a one-workgroup tail folds the B rows into five device scalars.  Nothing comes back to
// the host.  Top-k hits are decided by RANK: the best positive is among the k largest logits of
// its row iff fewer than k logits are strictly greater (ties go to the positive, as a stable
// descending sort would place the lower column first for column 0).
#include "common.h"
#include "../../include/coclr_hip.h"
#include <math.h>

namespace {

__device__ __forceinline__ float block256_max(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// row statistics: float[8] = {loss, lse, aux, lse_lo, aux_lo, 0, 0, rowmax}
//   aux = modes 0/1: log-sum-exp over the positives used by the loss; mode 2: their number.
//   lse_lo / aux_lo: on WIDE rows (below) what the fp32 rounding of lse / aux (a maximum plus a small logarithm)
//   dropped, so that the backward's exp(v - lse) and exp(v - aux) keep their relative accuracy when the logits are
//   large: lse + lse_lo == rowmax + log(sum exp(v - rowmax)) to the accuracy of the logarithm alone.  0 otherwise.
// A row is WIDE when |rowmax| >= 64 or its best positive lies 64 or more below rowmax.  Up to there the plain forms
// lse - lsp and exp(v - lse) are good to half an ulp of 128 (3.8e-6, inside the backward's 1e-5) and exp(v - rowmax)
// of a positive is a normal fp32 number (exp(-64) = 1.6e-28), and they are kept bit for bit: unit-norm features give
// |logit| <= 1 / T, so training never leaves them.  Beyond, exp(v - rowmax) of every positive can underflow (log(0):
// an infinite loss where the loss is finite) and the rounding of lse becomes the error of the gradient.
// flags[b] bit 0: column 0 was dropped from this row's loss mask (mode 1, drop_self);
//          bits 1..4: hit@k1, hit@k2, self hit@k1, self hit@k2.
__global__ void __launch_bounds__(256)
nce_loss_rows_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ mask,
                     const int64_t* __restrict__ target, float* __restrict__ rowstats,
                     uint8_t* __restrict__ flags, int N1, int mode, int drop_self, int k1, int k2) {
  __shared__ float redf[4];
  __shared__ double redd[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (long)b * N1;
  const uint8_t* mrow = mask ? mask + (long)b * N1 : nullptr;
  const int tcol = mode == 0 ? (int)target[b] : 0;

  // pass 1: row max, best positive, number of positives
  float vmax = -INFINITY, pmax = -INFINITY, pmax_rest = -INFINITY;   // _rest: positives other than column 0
  int npos = 0;
  for (int j = tid; j < N1; j += 256) {
    const float v = row[j];
    vmax = fmaxf(vmax, v);
    const bool pos = mode == 0 ? (j == tcol) : (mrow[j] != 0);
    if (pos) { pmax = fmaxf(pmax, v); ++npos; }
    if (pos && j > 0) pmax_rest = fmaxf(pmax_rest, v);
  }
  vmax = block256_max(vmax, redf);
  pmax = block256_max(pmax, redf);
  pmax_rest = block256_max(pmax_rest, redf);
  const int npos_all = (int)(block256_sum_d((double)npos, redd) + 0.5);
  const float l0 = row[0];
  const bool drop0 = mode == 1 && drop_self && npos_all != 1 && mrow[0] != 0;
  // wide rows: the positives' exp-sum is taken against THEIR maximum, not the row's
  const float lmax = drop0 ? pmax_rest : pmax;
  const bool wide = fabsf(vmax) >= 64.f || !(vmax - lmax < 64.f);

  // pass 2: exp sums and rank counts
  double se = 0.0, pe = 0.0, ps = 0.0;
  int gt_p = 0, gt_0 = 0;
  for (int j = tid; j < N1; j += 256) {
    const float v = row[j];
    const float e = expf(v - vmax);
    se += e;
    bool pos = mode == 0 ? (j == tcol) : (mrow[j] != 0);
    if (drop0 && j == 0) pos = false;
    if (pos) { pe += wide ? expf(v - lmax) : e; ps += v; }
    gt_p += v > pmax;
    gt_0 += v > l0;
  }
  se = block256_sum_d(se, redd);
  pe = block256_sum_d(pe, redd);
  ps = block256_sum_d(ps, redd);
  const int cgp = (int)(block256_sum_d((double)gt_p, redd) + 0.5);
  const int cg0 = (int)(block256_sum_d((double)gt_0, redd) + 0.5);
  if (tid == 0) {
    // wide rows form the loss from the DIFFERENCES (of the maxima, of the logs): lse - lsp would carry the rounding
    // of two numbers of the logits' magnitude into a loss that may be far smaller
    const float lz = logf((float)se);
    const float lse = vmax + lz;
    const int npos_eff = npos_all - (drop0 ? 1 : 0);
    float loss, aux, aux_lo = 0.f;
    if (mode == 2) {            // -(sum_pos log_softmax) / n_pos
      aux = (float)npos_eff;
      loss = wide ? (float)((double)vmax - ps / (double)npos_eff) + lz : lse - (float)(ps / (double)npos_eff);
    } else if (wide) {          // -log(sum_pos softmax); mode 0 is the one-positive case
      const float lp = logf((float)pe);
      aux = lmax + lp;
      aux_lo = (lmax - aux) + lp;
      loss = (vmax - lmax) + (lz - lp);
    } else {
      const float lsp = vmax + logf((float)pe);
      aux = lsp;
      loss = lse - lsp;
    }
    float* o = rowstats + 8 * (long)b;
    o[0] = loss; o[1] = lse; o[2] = aux;
    o[3] = wide ? (vmax - lse) + lz : 0.f; o[4] = aux_lo;
    o[5] = 0.f; o[6] = 0.f;
    o[7] = vmax;
    flags[b] = (uint8_t)((drop0 ? 1 : 0) | (cgp < k1 ? 2 : 0) | (cgp < k2 ? 4 : 0) | (cg0 < k1 ? 8 : 0) |
                         (cg0 < k2 ? 16 : 0));
  }
}

// scalars[0..4] = mean over rows of {loss, hit@k1, hit@k2, self hit@k1, self hit@k2}
__global__ void __launch_bounds__(256)
nce_loss_fold_kernel(const float* __restrict__ rowstats, const uint8_t* __restrict__ flags,
                     float* __restrict__ scalars, int B) {
  __shared__ double red[4];
  for (int f = 0; f < 5; ++f) {
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) s += f == 0 ? rowstats[8 * (long)b] : (float)((flags[b] >> f) & 1);
    s = block256_sum_d(s, red);
    if (threadIdx.x == 0) scalars[f] = (float)(s / B);
  }
}

// dlogits[b][j] = dloss/B * (softmax_j - w_j)
__global__ void __launch_bounds__(256)
nce_loss_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ mask,
                    const int64_t* __restrict__ target, const float* __restrict__ rowstats,
                    const uint8_t* __restrict__ flags, const float* __restrict__ dloss,
                    float* __restrict__ dlogits, int B, int N1, int mode) {
  const int b = blockIdx.y;
  const float* st = rowstats + 8 * (long)b;
  const float lse = st[1], aux = st[2], lse_lo = st[3], aux_lo = st[4];
  const float gs = dloss[0] / (float)B;
  const bool drop0 = (flags[b] & 1) != 0;
  const int tcol = mode == 0 ? (int)target[b] : 0;
  const float* row = logits + (long)b * N1;
  const uint8_t* mrow = mask ? mask + (long)b * N1 : nullptr;
  float* drow = dlogits + (long)b * N1;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < N1; j += gridDim.x * 256) {
    const float v = row[j];
    float w = 0.f;
    if (mode == 0) {
      w = j == tcol ? 1.f : 0.f;
    } else if (mrow[j] != 0 && !(drop0 && j == 0)) {
      w = mode == 1 ? expf((v - aux) - aux_lo) : 1.f / aux;
    }
    drow[j] = gs * (expf((v - lse) - lse_lo) - w);
  }
}

}  // namespace

extern "C" int coclr_nce_loss_fwd(const float* logits, const uint8_t* mask, const int64_t* target,
                                  float* rowstats, uint8_t* flags, float* scalars, int B, int N1,
                                  int mode, int drop_self, int k1, int k2, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || N1 <= 0 || mode < 0 || mode > 2 || k1 < 1 || k2 < 1) return COCLR_EINVAL;
  if ((mode == 0 && !target) || (mode != 0 && !mask)) return COCLR_EINVAL;
  if (!rowstats || !flags || !scalars) return COCLR_EINVAL;
  hipLaunchKernelGGL(nce_loss_rows_kernel, dim3(B), dim3(256), 0, stream, logits, mask, target,
                     rowstats, flags, N1, mode, drop_self, k1, k2);
  COCLR_LAUNCH_CHECK();
  hipLaunchKernelGGL(nce_loss_fold_kernel, dim3(1), dim3(256), 0, stream, rowstats, flags, scalars, B);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_nce_loss_bwd(const float* logits, const uint8_t* mask, const int64_t* target,
                                  const float* rowstats, const uint8_t* flags, const float* dloss,
                                  float* dlogits, int B, int N1, int mode, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || N1 <= 0 || mode < 0 || mode > 2) return COCLR_EINVAL;
  if ((mode == 0 && !target) || (mode != 0 && !mask)) return COCLR_EINVAL;
  int gx = cdiv(N1, 256 * 4);
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(nce_loss_bwd_kernel, dim3(gx, B), dim3(256), 0, stream, logits, mask, target,
                     rowstats, flags, dloss, dlogits, B, N1, mode);
  COCLR_LAUNCH_CHECK();
  return 0;
}
