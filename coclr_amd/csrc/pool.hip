// MaxPool3d (floor mode, -inf padding, first-max-wins like ATen) with argmax
// indices, its gather-style backward, and the global average pool of the
// projection head.  Replaces ATen max_pool3d_with_indices(+_backward) used at
// backbone/s3dg.py:105,151,162,173,190 / backbone/resnet_2d3d.py:141 and
// adaptive_avg_pool3d((1,1,1)) at model/pretrain.py:51.
//
// HBM-bound stencil kernels: one lane per output (forward) / per input
// (backward, no atomics -> deterministic), w fastest so a wave touches
// contiguous rows.
#include "common.h"
#include "../../include/coclr_hip.h"
#include <math.h>
#include <cstdlib>

namespace {

struct PoolGeom {
  int N, C;
  int Ti, Hi, Wi, To, Ho, Wo;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
  long x_nstride, y_nstride;   // floats between samples (channel slices allowed)
  // optional transform of the INPUT, applied as it is read: x' = x*in_scale[c] + in_shift[c], then
  // max(x', 0) when in_relu -- the BatchNorm+ReLU that precedes the pool (backbone/s3dg.py:60-64
  // then :151,162; the block outputs before :173,190), so the normalised tensor is never written
  const float* in_scale;
  const float* in_shift;
  int in_relu;
  int C0;                      // channels before T was folded into the plane count
  int tfold;
  int nt;                      // stream the big operand with non-temporal loads / stores (ld4 / st4, nt_bytes)
};

__device__ __forceinline__ float pool_in(const PoolGeom& g, float v, int c) {
  if (g.in_scale) {
    v = fmaf(v, g.in_scale[c], g.in_shift[c]);
    if (g.in_relu) v = fmaxf(v, 0.f);
  }
  return v;
}

// floor(n / d) for n >= 0 and a divisor that is the same in every lane: the tiled kernels turn a flat work-item
// number into (volume, t, h, w) and a plane number into (sample, channel) with run-time extents, and hipcc's
// 32-bit division is ~30 vector instructions each time -- more than the window scan it feeds.  Below 2^20 the
// quotient is a float multiply by the reciprocal (formed once per divisor) and one correction step: n is exact in
// fp32, and with 1 / d up to 2 ulp off and the product rounded once the product is within n / d * 2^-21 <= 1/2 of
// n / d, so its truncation is within one of the quotient.  Same value as n / d for every n.
struct PoolDiv { int d; float r; };
__device__ __forceinline__ PoolDiv pool_div(int d) {
  PoolDiv p;
  p.d = d;
  p.r = 1.f / (float)d;
  return p;
}
// n < 2^20 is the caller's: element and work-item numbers inside one workgroup's <= kTileFloats tile
__device__ __forceinline__ int pool_quot_small(int n, const PoolDiv& p) {
  int q = (int)((float)n * p.r);
  const int rem = n - q * p.d;
  q += (rem >= p.d ? 1 : 0) - (rem < 0 ? 1 : 0);
  return q;
}
// plane numbers: any n >= 0
__device__ __forceinline__ int pool_quot(int n, const PoolDiv& p) {
  if (n >= (1 << 20)) return n / p.d;
  return pool_quot_small(n, p);
}

// Volumes smaller than one pass of the workgroup (Si < 1024: fewer than 256 float4 slots) are staged and stored as
// ONE run of float4 slots over the group's tile, [gcount][S4], four slots per thread at a time -- every thread busy
// and its loads in flight together -- instead of volume by volume with part of the workgroup idle.  Slot e: i = the
// slot inside its volume, (n, c) = sample and plane of that volume.  Larger volumes keep the per-volume loop, whose
// plane arithmetic is scalar: the kernels are bound by vector instruction issue, and the ~45 per slot of this form
// cost more there than the round trips they overlap (MaxPool_3a forward 173 -> 187 us with it, MaxPool_5a 23 -> 18).
constexpr int kSlotRunBelow = 256;
struct PoolSlots { int S4, C, pl0; PoolDiv dS4, dC; };
__device__ __forceinline__ PoolSlots pool_slots(int S4, int C, int pl0) {
  PoolSlots s;
  s.S4 = S4; s.C = C; s.pl0 = pl0;
  s.dS4 = pool_div(S4); s.dC = pool_div(C);
  return s;
}
__device__ __forceinline__ void pool_slot(const PoolSlots& s, int e, int& i, int& n, int& c) {
  const int gi = pool_quot_small(e, s.dS4);
  i = e - gi * s.S4;
  const int pl = s.pl0 + gi;
  n = pool_quot(pl, s.dC);
  c = pl - n * s.C;
}

__global__ void __launch_bounds__(256)
maxpool3d_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int* __restrict__ idx,
                     const PoolGeom g) {
  const int So = g.To * g.Ho * g.Wo, Si = g.Ti * g.Hi * g.Wi;
  const int planes = g.N * g.C;
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const int n = pl / g.C, c = pl - n * g.C;
    const float* xp = x + (long)n * g.x_nstride + (long)c * Si;
    float* yp = y + (long)n * g.y_nstride + (long)c * So;
    int* ip = idx ? idx + (long)pl * So : nullptr;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < So; o += gridDim.x * 256) {
      const int ow = o % g.Wo;
      const int q = o / g.Wo;
      const int oh = q % g.Ho, ot = q / g.Ho;
      int t0 = ot * g.st - g.pt, h0 = oh * g.sh - g.ph, w0 = ow * g.sw - g.pw;
      const int t1 = min(t0 + g.kt, g.Ti), h1 = min(h0 + g.kh, g.Hi), w1 = min(w0 + g.kw, g.Wi);
      t0 = max(t0, 0); h0 = max(h0, 0); w0 = max(w0, 0);
      float best = -INFINITY;
      int bi = (t0 * g.Hi + h0) * g.Wi + w0;
      for (int t = t0; t < t1; ++t)
        for (int h = h0; h < h1; ++h)
          for (int w = w0; w < w1; ++w) {
            const int ii = (t * g.Hi + h) * g.Wi + w;
            const float v = pool_in(g, xp[ii], c);
            if (v > best || v != v) { best = v; bi = ii; }
          }
      yp[o] = best;
      if (ip) ip[o] = bi;
    }
  }
}

// smallest o with o*s > a  (a = i + pad - k)
__device__ __forceinline__ int first_out(int a, int s) { return a < 0 ? 0 : a / s + 1; }

// dx[i] (+)= sum over outputs whose window holds i and whose argmax == i.
__global__ void __launch_bounds__(256)
maxpool3d_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ idx, float* dx,
                     const PoolGeom g, long dy_nstride, long dx_nstride, int accumulate) {
  const int So = g.To * g.Ho * g.Wo, Si = g.Ti * g.Hi * g.Wi;
  const int planes = g.N * g.C;
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const int n = pl / g.C, c = pl - n * g.C;
    const float* dyp = dy + (long)n * dy_nstride + (long)c * So;
    const int* ip = idx + (long)pl * So;
    float* dxp = dx + (long)n * dx_nstride + (long)c * Si;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Si; i += gridDim.x * 256) {
      const int iw = i % g.Wi;
      const int q = i / g.Wi;
      const int ih = q % g.Hi, it = q / g.Hi;
      // outputs o with o*s - p <= i < o*s - p + k
      const int ot0 = first_out(it + g.pt - g.kt, g.st);
      const int oh0 = first_out(ih + g.ph - g.kh, g.sh);
      const int ow0 = first_out(iw + g.pw - g.kw, g.sw);
      const int ot1 = min(g.To - 1, (it + g.pt) / g.st);
      const int oh1 = min(g.Ho - 1, (ih + g.ph) / g.sh);
      const int ow1 = min(g.Wo - 1, (iw + g.pw) / g.sw);
      float s = 0.f;
      for (int ot = ot0; ot <= ot1; ++ot)
        for (int oh = oh0; oh <= oh1; ++oh)
          for (int ow = ow0; ow <= ow1; ++ow) {
            const int o = (ot * g.Ho + oh) * g.Wo + ow;
            if (ip[o] == i) s += dyp[o];
          }
      dxp[i] = accumulate ? dxp[i] + s : s;
    }
  }
}

// ---------------------------------------------------------------------------
// LDS-tiled pooling for the configurations the backbones use.  One workgroup
// owns G whole (n, c) input volumes (<= 16384 floats together): the volume is
// read from HBM exactly once with coalesced loads, the window scan runs out of
// LDS with a compile-time stencil, each lane produces WPT adjacent outputs of
// one row so every LDS row segment is read once per WPT outputs.
// ---------------------------------------------------------------------------
template <int KT, int KH, int KW, int ST, int SH, int SW, int WPT, bool WITH_IDX>
__global__ void __launch_bounds__(256)
maxpool3d_tiled_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                           int* __restrict__ idx, const PoolGeom g, int G, int planes, int tfold,
                           int vec) {
  extern __shared__ float tile[];   // [G][Si]
  const int Si = g.Ti * g.Hi * g.Wi, So = g.To * g.Ho * g.Wo;
  const int pl0 = blockIdx.x * G;
  const int gcount = min(G, planes - pl0);
  const PoolDiv dC = pool_div(g.C), dfold = pool_div(tfold);
  // ---- load: G volumes are contiguous per sample only if they share n; handle generally
  const int S4 = Si >> 2;
  if (vec && S4 < kSlotRunBelow) {      // PoolFwdPlan::vec: Si % 4 == 0 and x_nstride % 4 == 0
    const int total4 = gcount * S4;
    const PoolSlots slots = pool_slots(S4, g.C, pl0);
    for (int e0 = threadIdx.x; e0 < total4; e0 += 4 * 256) {
      float4 r[4];
      float sc[4], sf[4];             // the slot's channel coefficients, requested with its data
      bool live[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k * 256;
        live[k] = e < total4;
        sc[k] = sf[k] = 0.f;
        if (live[k]) {
          int i, n, c;
          pool_slot(slots, e, i, n, c);
          r[k] = ld4(x + (long)n * g.x_nstride + (long)c * Si, i, g.nt != 0);
          if (g.in_scale) {
            const int ch = pool_quot(c, dfold);   // channel of the un-folded tensor (g.tfold == tfold)
            sc[k] = g.in_scale[ch];
            sf[k] = g.in_shift[ch];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!live[k]) continue;
        float4 v = r[k];
        if (g.in_scale) {             // pool_in, with the coefficients already here
          v.x = fmaf(v.x, sc[k], sf[k]); v.y = fmaf(v.y, sc[k], sf[k]);
          v.z = fmaf(v.z, sc[k], sf[k]); v.w = fmaf(v.w, sc[k], sf[k]);
          if (g.in_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        }
        reinterpret_cast<float4*>(tile)[e0 + k * 256] = v;
      }
    }
  } else {
    for (int gi = 0; gi < gcount; ++gi) {
      const int pl = pl0 + gi;
      const int n = pool_quot(pl, dC), c = pl - n * g.C;
      const float* xp = x + (long)n * g.x_nstride + (long)c * Si;
      float* tp = tile + gi * Si;
      const int ch = pool_quot(c, dfold);  // channel of the un-folded tensor (g.tfold == tfold)
      if (vec) {
        for (int i = threadIdx.x; i < S4; i += 256) {
          float4 v = ld4(xp, i, g.nt != 0);
          v.x = pool_in(g, v.x, ch); v.y = pool_in(g, v.y, ch);
          v.z = pool_in(g, v.z, ch); v.w = pool_in(g, v.w, ch);
          reinterpret_cast<float4*>(tp)[i] = v;
        }
      } else {
        for (int i = threadIdx.x; i < Si; i += 256) tp[i] = pool_in(g, xp[i], ch);
      }
    }
  }
  __syncthreads();
  constexpr int NR = (WPT - 1) * SW + KW;    // input columns feeding WPT outputs
  const int OWC = (g.Wo + WPT - 1) / WPT;
  const int rows = g.To * g.Ho;
  const int items = gcount * rows * OWC;       // <= kTileFloats
  const PoolDiv dOWC = pool_div(OWC), dHo = pool_div(g.Ho), dTo = pool_div(g.To);
  for (int it = threadIdx.x; it < items; it += 256) {
    const int r0 = pool_quot_small(it, dOWC), owc = it - r0 * OWC;
    const int r1 = pool_quot_small(r0, dHo), oh = r0 - r1 * g.Ho;
    const int gi = pool_quot_small(r1, dTo), ot = r1 - gi * g.To;
    const int ow0 = owc * WPT;
    const float* tp = tile + gi * Si;
    float best[WPT];
    int bi[WPT];
    const int t0 = ot * ST - g.pt, h0 = oh * SH - g.ph, w0 = ow0 * SW - g.pw;
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      best[j] = -INFINITY;
      // ATen initialises argmax to the first in-range window element
      const int tt = max(t0, 0), hh = max(h0, 0), ww = max(w0 + j * SW, 0);
      bi[j] = (tt * g.Hi + hh) * g.Wi + ww;
    }
    // No branch around a row or a column outside the volume: every read goes to a clamped (valid) address and
    // the value is replaced by -inf, which the scan below never takes -- as skipping the element did.  All reads of
    // an item are then independent LDS loads with nothing but selects between them and the compares (the branchy
    // form waited for each read under its own exec mask).
    // (-inf through a register the optimiser cannot see into: knowing the constant, it turns every select back into a
    // branch around the read and the compares that -inf cannot win)
    float ninf = -INFINITY;
    asm volatile("" : "+v"(ninf));
    int wc[NR];
    bool wok[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      const int w = w0 + q;
      wok[q] = w >= 0 && w < g.Wi;
      wc[q] = min(max(w, 0), g.Wi - 1);
    }
    // at most 16 reads in flight: the three frames of a 3x3x3 window stay a loop (unrolled, their 45 to 54 reads
    // are all hoisted to the top and their registers halve the waves per SIMD)
#pragma unroll(KT * KH * NR <= 16 ? KT : 1)
    for (int kt = 0; kt < KT; ++kt) {
      const int t = t0 + kt;
      const bool tok = t >= 0 && t < g.Ti;
      const int tcl = min(max(t, 0), g.Ti - 1);
#pragma unroll
      for (int kh = 0; kh < KH; ++kh) {
        const int h = h0 + kh;
        const bool rok = tok && h >= 0 && h < g.Hi;
        const int rowoff = (t * g.Hi + h) * g.Wi;            // used only by elements that exist
        const float* rp = tp + (tcl * g.Hi + min(max(h, 0), g.Hi - 1)) * g.Wi;
        float v[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          const float e = rp[wc[q]];
          v[q] = (rok && wok[q]) ? e : ninf;
        }
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
#pragma unroll
          for (int kw = 0; kw < KW; ++kw) {
            const float val = v[j * SW + kw];
            if (val > best[j] || val != val) { best[j] = val; bi[j] = rowoff + w0 + j * SW + kw; }
          }
        }
      }
    }
    const int pl = pl0 + gi;
    const int n = pool_quot(pl, dC), c = pl - n * g.C;
    const long obase = ((long)ot * g.Ho + oh) * g.Wo + ow0;
    float* yp = y + (long)n * g.y_nstride + (long)c * So + obase;
    // indices are relative to the un-folded (n, c) volume
    const int fold_off = WITH_IDX ? (pl - pool_quot(pl, dfold) * tfold) * Si : 0;
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      if (ow0 + j < g.Wo) {
        yp[j] = best[j];
        if (WITH_IDX) idx[(long)pl * So + obase + j] = bi[j] + fold_off;
      }
    }
  }
}

// Backward: the G input-gradient volumes live in LDS; every output element adds its gradient to
// the input element it selected.  Run-to-run DETERMINISTIC and atomic-free: outputs are visited in
// ceil(k/s)^3 colour classes ((ot, oh, ow) mod ceil(k/s)); the windows of two outputs of one class
// are disjoint, so within a class the read-modify-writes cannot collide, and the classes run in a
// fixed order with a barrier in between -- every input element receives its <= 27 addends in the
// same order every time.  Then the tile is written (or accumulated) to HBM with coalesced stores.
// With the class counts known at compile time (PT, PH, PW > 0) and at most KQ outputs per thread and
// class, every (arg-max, dy) pair of the workgroup is loaded UP FRONT -- one global round trip instead
// of one per class (27 for the 3x3x3 / 1 pools) -- and the classes are then applied from registers
// with an LDS-only barrier in between.  Same addends in the same order as the generic form.
template <int PT, int PH, int PW, int KQ>
struct ClassLoads {
  int i[PT * PH * PW][KQ];      // the arg-max index AS LOADED (-1: no element), added to b only when applied:
  float v[PT * PH * PW][KQ];    // arithmetic on the loaded value next to the load would make every class wait
  int b[KQ];                    // for its own round trip before the next class's loads are even issued
};

// Thread slot q = threadIdx.x + k * 256 owns ONE block of PT x PH x PW neighbouring outputs of one volume, the
// output (a * PT + ct, b * PH + ch, cc * PW + cw) of every class (ct, ch, cw): the slot is taken apart into
// (volume, a, b, cc) once, and a class only adds its constant offset and tests that its output exists.  (Taking q
// apart per class, by that class's own extents, cost five 32-bit divisions per class and slot: 4063 vector
// instructions per thread in the 27-class form.)  Which lane holds which output of a class is free -- the windows
// of one class are disjoint -- so every input element still receives its addends in class order.
// class_shape's kq is the slot count per thread: G * ceil(To / PT) * ceil(Ho / PH) * ceil(Wo / PW) <= KQ * 256.
template <int PT, int PH, int PW, int KQ>
__device__ __forceinline__ void class_load(ClassLoads<PT, PH, PW, KQ>& L, const float* __restrict__ dy,
                                           const int* __restrict__ idx, const PoolGeom& g,
                                           long dy_nstride, int pl0, int gcount, int tfold, int Si,
                                           int So) {
  const int mt = (g.To + PT - 1) / PT, mh = (g.Ho + PH - 1) / PH, mw = (g.Wo + PW - 1) / PW;
  const int msize = mt * mh * mw;              // gcount * msize <= KQ * 256
  const PoolDiv dsize = pool_div(msize), dhw = pool_div(mh * mw), dw = pool_div(mw);
  const PoolDiv dC = pool_div(g.C), dfold = pool_div(tfold);
#pragma unroll
  for (int k = 0; k < KQ; ++k) {
    const int q = threadIdx.x + k * 256;
    const bool live = q < gcount * msize;
    const int gi = live ? pool_quot_small(q, dsize) : 0;
    int m = live ? q - gi * msize : 0;
    const int a = pool_quot_small(m, dhw);
    m -= a * mh * mw;
    const int b = pool_quot_small(m, dw), cc = m - b * mw;
    const int t0 = a * PT, h0 = b * PH, w0 = cc * PW;
    const int o0 = (t0 * g.Ho + h0) * g.Wo + w0;
    const int pl = pl0 + gi;
    const int n = pool_quot(pl, dC), c = pl - n * g.C;
    const int* ip = idx + (long)pl * So + o0;
    const float* dp = dy + (long)n * dy_nstride + (long)c * So + o0;
    L.b[k] = gi * Si - (pl - pool_quot(pl, dfold) * tfold) * Si;
#pragma unroll
    for (int ct = 0; ct < PT; ++ct)
#pragma unroll
      for (int ch = 0; ch < PH; ++ch)
#pragma unroll
        for (int cw = 0; cw < PW; ++cw) {
          const int cls = (ct * PH + ch) * PW + cw;
          const int off = (ct * g.Ho + ch) * g.Wo + cw;
          const bool has = live && t0 + ct < g.To && h0 + ch < g.Ho && w0 + cw < g.Wo;
          L.i[cls][k] = -1;
          L.v[cls][k] = 0.f;
          if (has) {
            L.i[cls][k] = ip[off];
            L.v[cls][k] = dp[off];
          }
        }
  }
}

// the tile's zero fill (or anything else written to LDS before) must be followed by no barrier of
// its own: the first class starts with one
template <int PT, int PH, int PW, int KQ>
__device__ __forceinline__ void class_apply(const ClassLoads<PT, PH, PW, KQ>& L, float* tile) {
#pragma unroll
  for (int cls = 0; cls < PT * PH * PW; ++cls) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS only: the loads stay in flight
#pragma unroll
    for (int k = 0; k < KQ; ++k)
      if (L.i[cls][k] >= 0) tile[L.b[k] + L.i[cls][k]] += L.v[cls][k];
  }
}

// generic form: class counts from the geometry, one global round trip per class
__device__ __forceinline__ void class_scatter_generic(float* tile, const float* __restrict__ dy,
                                                      const int* __restrict__ idx, const PoolGeom& g,
                                                      long dy_nstride, int pl0, int gcount, int tfold,
                                                      int Si, int So) {
  const int Pt = (g.kt + g.st - 1) / g.st, Ph = (g.kh + g.sh - 1) / g.sh, Pw = (g.kw + g.sw - 1) / g.sw;
  for (int ct = 0; ct < Pt; ++ct)
    for (int ch = 0; ch < Ph; ++ch)
      for (int cw = 0; cw < Pw; ++cw) {
        __syncthreads();
        const int nt = (g.To - ct + Pt - 1) / Pt, nh = (g.Ho - ch + Ph - 1) / Ph,
                  nw = (g.Wo - cw + Pw - 1) / Pw;
        if (nt <= 0 || nh <= 0 || nw <= 0) continue;       // uniform across the workgroup
        const int csize = nt * nh * nw;
        for (int q = threadIdx.x; q < gcount * csize; q += 256) {
          const int gi = q / csize;
          int m = q - gi * csize;
          const int a = m / (nh * nw);
          m -= a * nh * nw;
          const int b = m / nw, cc = m - b * nw;
          const int o = ((a * Pt + ct) * g.Ho + (b * Ph + ch)) * g.Wo + (cc * Pw + cw);
          const int pl = pl0 + gi;
          const int n = pl / g.C, c = pl - n * g.C;
          const int i = idx[(long)pl * So + o] - (pl % tfold) * Si;
          tile[gi * Si + i] += dy[(long)n * dy_nstride + (long)c * So + o];
        }
      }
}

template <int PT, int PH, int PW, int KQ>
__global__ void __launch_bounds__(256)
maxpool3d_tiled_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ idx, float* dx,
                           const PoolGeom g, long dy_nstride, long dx_nstride, int accumulate,
                           int G, int planes, int tfold, int vec) {
  extern __shared__ float tile[];   // [G][Si]
  const int Si = g.Ti * g.Hi * g.Wi, So = g.To * g.Ho * g.Wo;
  const int pl0 = blockIdx.x * G;
  const int gcount = min(G, planes - pl0);
  if constexpr (PT > 0) {
    ClassLoads<PT, PH, PW, KQ> L;
    class_load<PT, PH, PW, KQ>(L, dy, idx, g, dy_nstride, pl0, gcount, tfold, Si, So);
    for (int i = threadIdx.x; i < gcount * Si; i += 256) tile[i] = 0.f;
    class_apply<PT, PH, PW, KQ>(L, tile);
  } else {
    for (int i = threadIdx.x; i < gcount * Si; i += 256) tile[i] = 0.f;
    class_scatter_generic(tile, dy, idx, g, dy_nstride, pl0, gcount, tfold, Si, So);
  }
  __syncthreads();
  const PoolDiv dC = pool_div(g.C);
  const int S4 = Si >> 2;
  if (vec && S4 < kSlotRunBelow) {      // PoolBwdPlan::vec: Si % 4 == 0 and dx_nstride % 4 == 0
    const int total4 = gcount * S4;
    const PoolSlots slots = pool_slots(S4, g.C, pl0);
    for (int e0 = threadIdx.x; e0 < total4; e0 += 4 * 256) {
      float4 o[4];
      float* dp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k * 256;
        dp[k] = nullptr;
        if (e < total4) {
          int i, n, c;
          pool_slot(slots, e, i, n, c);
          dp[k] = dx + (long)n * dx_nstride + (long)c * Si + 4 * i;
          if (accumulate) o[k] = *reinterpret_cast<const float4*>(dp[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!dp[k]) continue;
        float4 v = reinterpret_cast<const float4*>(tile)[e0 + k * 256];
        if (accumulate) { v.x += o[k].x; v.y += o[k].y; v.z += o[k].z; v.w += o[k].w; }
        *reinterpret_cast<float4*>(dp[k]) = v;
      }
    }
    return;
  }
  for (int gi = 0; gi < gcount; ++gi) {
    const int pl = pl0 + gi;
    const int n = pool_quot(pl, dC), c = pl - n * g.C;
    float* dxp = dx + (long)n * dx_nstride + (long)c * Si;
    const float* tp = tile + gi * Si;
    if (vec) {
      for (int i = threadIdx.x; i < S4; i += 256) {
        float4 v = reinterpret_cast<const float4*>(tp)[i];
        if (accumulate) {
          const float4 o = reinterpret_cast<const float4*>(dxp)[i];
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        reinterpret_cast<float4*>(dxp)[i] = v;
      }
    } else {
      for (int i = threadIdx.x; i < Si; i += 256) dxp[i] = accumulate ? dxp[i] + tp[i] : tp[i];
    }
  }
}


// ---------------------------------------------------------------------------
// 3x3x3 / stride 1 / pad 1 (the pool branch of every inception block, backbone/s3dg.py:105) on
// small planes (H*W = 256, 64 or 16).  The 27-element scan with argmax tracking is VALU-bound
// (~110 operations per output); the maximum is separable, and so is "first maximum in (t, h, w)
// scan order": max over w, then over h, then over t, each stage keeping the earliest of equal
// values -- 6 combines per output instead of 26.  Thread = (volume, h, w); it walks t with a
// three-plane sliding window of in-plane maxima.  NaN handling and the initial argmax (first
// in-range element) are those of the scan above.
// ---------------------------------------------------------------------------
struct PoolBest { float v; int i; };

__device__ __forceinline__ void pool_take(PoolBest& b, float cv, int ci) {
  if (cv > b.v || cv != cv) { b.v = cv; b.i = ci; }
}

template <bool WITH_IDX, int TT>
__global__ void __launch_bounds__(256)
maxpool333_kernel(const float* __restrict__ x, float* __restrict__ y, int* __restrict__ idx,
                  const PoolGeom g, int planes, int lW, int lHW, int vec) {
  extern __shared__ float lds[];
  const int T = TT > 0 ? TT : g.Ti;                  // compile-time frame count: the t loops unroll
  const int W = 1 << lW, HW = 1 << lHW, H = HW >> lW;
  const int PG = 256 >> lHW, S = T << lHW;          // volumes per workgroup, floats per volume
  float* xs = lds;                                   // [PG][T][HW]
  float* bv = xs + PG * S;                           // w-stage maxima
  int* bi = reinterpret_cast<int*>(bv + PG * S);     // ... and their flat indices
  const int tid = threadIdx.x;
  const int pl0 = blockIdx.x * PG;
  const int gcount = min(PG, planes - pl0);
  if (vec) {        // PoolFwdPlan::vec: x_nstride % 4 == 0 (S is a multiple of 16)
    // [PG][S] is one run of <= 1024 float4 slots: all of a thread's loads in flight at once
    const int S4 = S >> 2, total4 = gcount * S4;
    for (int e0 = tid; e0 < total4; e0 += 4 * 256) {
      float4 r[4];
      int chn[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k * 256;
        chn[k] = -1;
        if (e < total4) {
          const int gi = e / S4, i = e - gi * S4;
          const int pl = pl0 + gi;
          const int n = pl / g.C, c = pl - n * g.C;
          r[k] = reinterpret_cast<const float4*>(x + (long)n * g.x_nstride + (long)c * S)[i];
          chn[k] = c;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (chn[k] < 0) continue;
        float4 v = r[k];
        v.x = pool_in(g, v.x, chn[k]); v.y = pool_in(g, v.y, chn[k]);
        v.z = pool_in(g, v.z, chn[k]); v.w = pool_in(g, v.w, chn[k]);
        reinterpret_cast<float4*>(xs)[e0 + k * 256] = v;
      }
    }
  } else {
    for (int gi = 0; gi < gcount; ++gi) {
      const int pl = pl0 + gi;
      const int n = pl / g.C, c = pl - n * g.C;
      const float* xp = x + (long)n * g.x_nstride + (long)c * S;
      float* tp = xs + gi * S;
      for (int i = tid; i < S; i += 256) tp[i] = pool_in(g, xp[i], c);
    }
  }
  __syncthreads();
  const int gl = tid >> lHW, p = tid & (HW - 1), h = p >> lW, w = p & (W - 1);
  const bool live = gl < gcount;
  // stage 1: along w
  if (live) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int row = (gl * T + t) * HW + h * W;
      const int frow = (t * H + h) * W;              // flat index of the row start in the volume
      PoolBest b;
      b.v = -INFINITY;
      b.i = frow + (w > 0 ? w - 1 : 0);
      if (w > 0) pool_take(b, xs[row + w - 1], frow + w - 1);
      pool_take(b, xs[row + w], frow + w);
      if (w < W - 1) pool_take(b, xs[row + w + 1], frow + w + 1);
      bv[row + w] = b.v;
      if (WITH_IDX) bi[row + w] = b.i;
    }
  }
  __syncthreads();
  if (!live) return;
  // stage 2 (along h) for one plane
  auto plane_best = [&](int t) {
    const int col = (gl * T + t) * HW + w;
    const int h0 = h > 0 ? h - 1 : 0;
    PoolBest b;
    b.v = -INFINITY;
    b.i = WITH_IDX ? bi[col + h0 * W] : 0;
    if (h > 0) pool_take(b, bv[col + (h - 1) * W], WITH_IDX ? bi[col + (h - 1) * W] : 0);
    pool_take(b, bv[col + h * W], WITH_IDX ? bi[col + h * W] : 0);
    if (h < H - 1) pool_take(b, bv[col + (h + 1) * W], WITH_IDX ? bi[col + (h + 1) * W] : 0);
    return b;
  };
  const int pl = pl0 + gl;
  const int n = pl / g.C, c = pl - n * g.C;
  float* yp = y + (long)n * g.y_nstride + (long)c * S;
  int* ip = WITH_IDX ? idx + (long)pl * S : nullptr;
  // stage 3: sliding window along t
  PoolBest prev, cur = plane_best(0), next = cur;
  prev.v = -INFINITY; prev.i = cur.i;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) next = plane_best(t + 1);
    PoolBest b;
    b.v = -INFINITY;
    b.i = t > 0 ? prev.i : cur.i;                  // first in-range element of the window
    if (t > 0) pool_take(b, prev.v, prev.i);
    pool_take(b, cur.v, cur.i);
    if (t + 1 < T) pool_take(b, next.v, next.i);
    yp[t * HW + p] = b.v;
    if (WITH_IDX) ip[t * HW + p] = b.i;
    prev = cur;
    cur = next;
  }
}

// ---------------------------------------------------------------------------
// BatchNorm(+ReLU) backward of a unit whose ONLY consumer is a max-pool that applied the affine +
// ReLU while reading (engine.max_pool, lazy apply: MaxPool_2a behind Conv_1a, MaxPool_3a behind
// Conv_2c).  The gradient dz of the normalised activation is then nothing but the pool's dy scattered
// to the arg-max positions, so it is never materialised:
//   reduce (output-centric): sum g and sum g*xhat over the pool OUTPUTS, g = dy_pool[o] masked by the
//           ReLU at y[argmax(o)]  -- reads the two quarter-size tensors and gathers y;
//   apply  (the pool-backward tile kernel with a BatchNorm epilogue): the plane's g in LDS (colour
//           classes, deterministic), then dy_bn = A*g*mask + B*y + D streamed out with y streamed in.
// Against pool backward + two-pass BatchNorm backward (6.5 |y| of traffic, three kernels) this moves
// about 4 |y| in two.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
bn_pool_bwd_reduce_kernel(const float* __restrict__ pdy, const int* __restrict__ pidx,
                          const float* __restrict__ y, const float* __restrict__ scale,
                          const float* __restrict__ shift, const float* __restrict__ mean,
                          const float* __restrict__ invstd, double* sums, int C, int So, int Si,
                          long pdy_nstride, long y_nstride, int relu) {
  __shared__ double red[4];
  const int c = blockIdx.x, n = blockIdx.y;
  const float sc = scale[c], sf = shift[c], mu = mean[c], is = invstd[c];
  const float* dp = pdy + (long)n * pdy_nstride + (long)c * So;
  const int* ip = pidx + ((long)n * C + c) * So;
  const float* yp = y + (long)n * y_nstride + (long)c * Si;
  float ag = 0.f, agx = 0.f;
  // four outputs per trip: the arg-max loads of all four, then the four dependent gathers of y -- two
  // round trips per four outputs instead of per output (same per-thread summation order)
  for (int o0 = threadIdx.x; o0 < So; o0 += 1024) {
    int ii[4];
    float gg[4], vv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = o0 + k * 256;
      ii[k] = o < So ? ip[o] : 0;
      gg[k] = o < So ? dp[o] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) vv[k] = yp[ii[k]];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (o0 + k * 256 >= So) break;
      float g = gg[k];
      const float v = vv[k];
      if (relu) g = fmaf(v, sc, sf) > 0.f ? g : 0.f;
      ag += g;
      agx += g * ((v - mu) * is);
    }
  }
  double sg = block256_sum_d((double)ag, red);
  double sgx = block256_sum_d((double)agx, red);
  if (threadIdx.x == 0) {
    sums[((long)c * gridDim.y + n) * 2] = sg;
    sums[((long)c * gridDim.y + n) * 2 + 1] = sgx;
  }
}

template <int PT, int PH, int PW, int KQ>
__global__ void __launch_bounds__(256)
bn_pool_bwd_apply_kernel(const float* __restrict__ pdy, const int* __restrict__ pidx,
                         const float* __restrict__ y, const float* __restrict__ scale,
                         const float* __restrict__ shift, const float* __restrict__ mean,
                         const float* __restrict__ invstd, const double* __restrict__ sums, int groups,
                         double count, int training, float* dgamma, float* dbeta, float* dy,
                         const PoolGeom g, long pdy_nstride, long y_nstride, long dy_nstride, int relu,
                         int G, int planes, int tfold, int vec) {
  extern __shared__ float tile[];   // [G][Si]
  __shared__ double tot[2];
  __shared__ float coef[8][4];      // per volume of the group: A, B, D, (unused)
  const int Si = g.Ti * g.Hi * g.Wi, So = g.To * g.Ho * g.Wo;
  const int pl0 = blockIdx.x * G;
  const int gcount = min(G, planes - pl0);
  ClassLoads<(PT > 0 ? PT : 1), (PT > 0 ? PH : 1), (PT > 0 ? PW : 1), (PT > 0 ? KQ : 1)> L;
  if constexpr (PT > 0)           // in flight while the coefficients are formed
    class_load<PT, PH, PW, KQ>(L, pdy, pidx, g, pdy_nstride, pl0, gcount, tfold, Si, So);
  for (int i = threadIdx.x; i < gcount * Si; i += 256) tile[i] = 0.f;
  // coefficients of the channels this group touches (g.C counts folded planes: channel = (pl % C) /
  // tfold); neighbouring planes of a folded volume share their channel's
  int cprev = -1;
  for (int gi = 0; gi < gcount; ++gi) {
    const int pl = pl0 + gi;
    const int c = (pl % g.C) / tfold;
    if (c == cprev && !(pl / g.C == 0 && (pl % g.C) % tfold == 0)) {      // uniform
      if (threadIdx.x == 0)       // the thread that wrote them
        for (int j = 0; j < 3; ++j) coef[gi][j] = coef[gi - 1][j];
      continue;
    }
    cprev = c;
    __syncthreads();
    if (threadIdx.x < 64) {
      double a0 = 0.0, a1 = 0.0;
      for (int k = threadIdx.x; k < groups; k += 64) {
        a0 += sums[((long)c * groups + k) * 2];
        a1 += sums[((long)c * groups + k) * 2 + 1];
      }
      a0 = wave_sum_d(a0);
      a1 = wave_sum_d(a1);
      if (threadIdx.x == 0) { tot[0] = a0; tot[1] = a1; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double sg = tot[0], sgx = tot[1];
      const float sc = scale[c];
      float A = sc, B = 0.f, D = 0.f;
      if (training) {
        const float mg = (float)(sg / count), mgx = (float)(sgx / count);
        B = -sc * invstd[c] * mgx;
        D = sc * (mean[c] * invstd[c] * mgx - mg);
      }
      coef[gi][0] = A; coef[gi][1] = B; coef[gi][2] = D;
      // the plane (sample 0, frame 0) of a channel also emits its dgamma / dbeta
      if (pl / g.C == 0 && (pl % g.C) % tfold == 0) {
        if (dgamma) dgamma[c] = (float)sgx;
        if (dbeta) dbeta[c] = (float)sg;
      }
    }
  }
  if constexpr (PT > 0) class_apply<PT, PH, PW, KQ>(L, tile);
  else class_scatter_generic(tile, pdy, pidx, g, pdy_nstride, pl0, gcount, tfold, Si, So);
  __syncthreads();
  const PoolDiv dC = pool_div(g.C), dfold = pool_div(tfold);
  for (int gi = 0; gi < gcount; ++gi) {
    const int pl = pl0 + gi;
    const int n = pool_quot(pl, dC), c = pl - n * g.C;       // c: folded plane index inside the sample
    const int ch = pool_quot(c, dfold);
    const float A = coef[gi][0], B = coef[gi][1], D = coef[gi][2];
    const float sc = scale[ch], sf = shift[ch];
    const float* yp = y + (long)n * y_nstride + (long)c * Si;
    float* dyp = dy + (long)n * dy_nstride + (long)c * Si;
    const float* tp = tile + gi * Si;
    if (vec) {      // PooledBnPlan::vec: Si % 4 == 0 and y_nstride, dy_nstride % 4 == 0
      for (int i = threadIdx.x; i < (Si >> 2); i += 256) {
        float4 gq = reinterpret_cast<const float4*>(tp)[i];
        const float4 v = ld4(yp, i, g.nt != 0);
        if (relu) {
          gq.x = fmaf(v.x, sc, sf) > 0.f ? gq.x : 0.f; gq.y = fmaf(v.y, sc, sf) > 0.f ? gq.y : 0.f;
          gq.z = fmaf(v.z, sc, sf) > 0.f ? gq.z : 0.f; gq.w = fmaf(v.w, sc, sf) > 0.f ? gq.w : 0.f;
        }
        float4 o;
        o.x = fmaf(A, gq.x, fmaf(B, v.x, D)); o.y = fmaf(A, gq.y, fmaf(B, v.y, D));
        o.z = fmaf(A, gq.z, fmaf(B, v.z, D)); o.w = fmaf(A, gq.w, fmaf(B, v.w, D));
        st4(dyp, i, o, g.nt != 0);
      }
    } else {
      for (int i = threadIdx.x; i < Si; i += 256) {
        float gv = tp[i];
        const float v = yp[i];
        if (relu) gv = fmaf(v, sc, sf) > 0.f ? gv : 0.f;
        dyp[i] = fmaf(A, gv, fmaf(B, v, D));
      }
    }
  }
}

// Backward of the 3x3x3 / stride 1 / pad 1 pool, GATHER form: dy and the argmax indices of G whole
// volumes are staged in LDS, thread i sums dy[o] over the <= 27 outputs o whose window holds input i
// and whose argmax is i, in fixed (t, h, w) order: no atomics, run-to-run deterministic, every
// thread busy (the scatter form has 27 colour classes of S/27 outputs each).
__global__ void __launch_bounds__(256)
maxpool333_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ idx, float* dx,
                      const PoolGeom g, long dy_nstride, long dx_nstride, int accumulate, int G,
                      int planes, int lW, int lHW, int vec) {
  extern __shared__ float lds[];
  const int T = g.Ti, W = 1 << lW, HW = 1 << lHW, H = HW >> lW;
  const int S = T << lHW;
  float* dys = lds;                                  // [G][S]
  int* ids = reinterpret_cast<int*>(lds + G * S);    // [G][S]
  const int pl0 = blockIdx.x * G;
  const int gcount = min(G, planes - pl0);
  for (int gi = 0; gi < gcount; ++gi) {
    const int pl = pl0 + gi;
    const int n = pl / g.C, c = pl - n * g.C;
    const float* dyp = dy + (long)n * dy_nstride + (long)c * S;
    const int* ip = idx + (long)pl * S;
    // PoolBwdPlan::vec: 16-byte staging needs whole float4 slots per volume, (S & 3) == 0 as well as
    // (dy_nstride & 3) == 0: with S % 4 != 0 (H*W = 1 or 2 and few frames) the last S % 4 elements would stay
    // unstaged and dyp / ip sit off 16 bytes for odd planes
    if (vec) {
      for (int i = threadIdx.x; i < (S >> 2); i += 256) {
        reinterpret_cast<float4*>(dys + gi * S)[i] = reinterpret_cast<const float4*>(dyp)[i];
        reinterpret_cast<int4*>(ids + gi * S)[i] = reinterpret_cast<const int4*>(ip)[i];
      }
    } else {
      for (int i = threadIdx.x; i < S; i += 256) { dys[gi * S + i] = dyp[i]; ids[gi * S + i] = ip[i]; }
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < gcount * S; q += 256) {
    const int gi = q / S, i = q - gi * S;
    const int t = i >> lHW, h = (i >> lW) & (H - 1), w = i & (W - 1);
    const float* dv = dys + gi * S;
    const int* iv = ids + gi * S;
    float s = 0.f;
#pragma unroll
    for (int dt = -1; dt <= 1; ++dt) {
      if (t + dt < 0 || t + dt >= T) continue;
#pragma unroll
      for (int dh = -1; dh <= 1; ++dh) {
        if (h + dh < 0 || h + dh >= H) continue;
#pragma unroll
        for (int dw = -1; dw <= 1; ++dw) {
          if (w + dw < 0 || w + dw >= W) continue;
          const int o = i + dt * HW + dh * W + dw;
          if (iv[o] == i) s += dv[o];
        }
      }
    }
    const int pl = pl0 + gi;
    const int n = pl / g.C, c = pl - n * g.C;
    float* d = dx + (long)n * dx_nstride + (long)c * S + i;
    *d = accumulate ? *d + s : s;
  }
}

constexpr int kTileFloats = 16384;   // 64 KiB of LDS per workgroup

// Volumes per workgroup of an LDS-tiled kernel: what `budget` floats of LDS hold (at least one, at most `cap` when
// given), halved while that leaves fewer than `min_wgs` workgroups.
inline int volumes_per_wg(int planes, int Si, int budget, int min_wgs, int cap = 0) {
  int G = budget / Si;
  if (G < 1) G = 1;
  if (cap > 0 && G > cap) G = cap;
  while (G > 1 && (planes + G - 1) / G < min_wgs) G >>= 1;
  return G;
}

// Collapse T into the plane count when the stencil does not touch it.
inline PoolGeom fold_time(PoolGeom g) {
  if (g.kt == 1 && g.st == 1 && g.pt == 0 && g.Ti == g.To) {
    // (n, c, t) volumes of H*W: only valid when samples are dense in (C,T,H,W), which
    // holds for channel-slice views as long as C*T planes of one sample are contiguous
    g.C = g.C * g.Ti;
    g.tfold = g.Ti;
    g.Ti = g.To = 1;
  }
  return g;
}

// y[n][c] = mean over S contiguous elements; one wave per (n, c).
__global__ void __launch_bounds__(256)
global_avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int planes, int S) {
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= planes) return;
  const float* xp = x + (long)wave * S;
  float s = 0.f;
  for (int i = lane; i < S; i += 64) s += xp[i];
  s = wave_sum(s);
  if (lane == 0) y[wave] = s / (float)S;
}

__global__ void __launch_bounds__(256)
global_avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long total, int S) {
  const float inv = 1.f / (float)S;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
    dx[e] = dy[e / S] * inv;
}

inline dim3 pool_grid(int planes, int elems) {
  int gx = cdiv(elems, 256 * 2);
  if (gx < 1) gx = 1;
  if (gx > 128) gx = 128;
  int gy = planes > 65535 ? 65535 : planes;
  while ((long)gx * gy > 262144 && gx > 1) gx >>= 1;
  return dim3(gx, gy);
}

inline PoolGeom to_geom(const coclr_pool_desc* d) {
  PoolGeom g;
  g.N = d->N; g.C = d->C;
  g.Ti = d->Ti; g.Hi = d->Hi; g.Wi = d->Wi; g.To = d->To; g.Ho = d->Ho; g.Wo = d->Wo;
  g.kt = d->kt; g.kh = d->kh; g.kw = d->kw; g.st = d->st; g.sh = d->sh; g.sw = d->sw;
  g.pt = d->pt; g.ph = d->ph; g.pw = d->pw;
  g.x_nstride = d->x_nstride; g.y_nstride = d->y_nstride;
  g.in_scale = g.in_shift = nullptr; g.in_relu = 0; g.C0 = d->C; g.tfold = 1;
  static const long nt_from = nt_bytes();
  g.nt = (nt_from >= 0 && (long)d->N * d->C * d->Ti * d->Hi * d->Wi * 4 >= nt_from) ? 1 : 0;
  return g;
}

inline int ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

inline bool is_333_s1_p1(const PoolGeom& g) {
  return g.kt == 3 && g.kh == 3 && g.kw == 3 && g.st == 1 && g.sh == 1 && g.sw == 1 && g.pt == 1 && g.ph == 1 &&
         g.pw == 1;
}

// ---------------------------------------------------------------------------
// Dispatch.  Each kernel family has ONE table; a row is one instantiation, built by a *_row<...>() template from a
// single spelling of the template arguments: the numbers coclr_pool_plan reports about it and the function that
// launches it.  A plan_* function picks the row and the launch numbers from the geometry; the entry points are
// validate, plan, row->launch, and coclr_pool_plan reports the same plan structs and rows without launching, so the
// tests' view of "which kernel does this shape reach" is the launchers' own.
// ---------------------------------------------------------------------------
enum { kFwdGeneric = 0, kFwdSep333 = 1, kFwdTiled = 2 };
enum { kBwdGeneric = 0, kBwdGather333 = 1, kBwdClasses = 2 };

// ---- forward ----------------------------------------------------------------------------------------------------
struct PoolFwdPlan;
typedef int (*PoolFwdFn)(const PoolFwdPlan&, const float* x, float* y, int32_t* idx, hipStream_t);

struct PoolFwdPlan {
  int family;        // kFwd*
  int tmpl;          // separable: TT (0: run-time frame count); tiled: row of kTiledFwd; generic: 0
  int G;             // volumes per workgroup (PG of the separable kernel)
  int gx, gy;        // grid
  int tfold;
  int vec;           // 16-byte staging of x
  int lds;           // dynamic LDS bytes
  int lW, lHW;       // separable kernel only
  int planes;        // (folded) volumes
  PoolGeom g;        // the geometry the kernel gets (T folded into the planes for the tiled family)
  const PoolFwdFn* launch;   // the row's launch functions {without, with indices}; nullptr: the generic kernel
};

template <auto Kern>
int launch_tiled_fwd(const PoolFwdPlan& p, const float* x, float* y, int32_t* idx, hipStream_t st) {
  return launch_dyn_lds<Kern, 256, kTileFloats * 4>(dim3(p.gx), (size_t)p.lds, st, x, y, idx, p.g, p.G, p.planes,
                                                    p.tfold, p.vec);
}

template <auto Kern>
int launch_sep333(const PoolFwdPlan& p, const float* x, float* y, int32_t* idx, hipStream_t st) {
  hipLaunchKernelGGL(Kern, dim3(p.gx), dim3(256), (size_t)p.lds, st, x, y, idx, p.g, p.planes, p.lW, p.lHW, p.vec);
  COCLR_LAUNCH_CHECK();
  return 0;
}

struct TiledFwdRow { int kt, kh, kw, st, sh, sw, wpt; PoolFwdFn launch[2]; };
template <int KT, int KH, int KW, int ST, int SH, int SW, int WPT>
constexpr TiledFwdRow tiled_fwd_row() {
  return {KT, KH, KW, ST, SH, SW, WPT,
          {&launch_tiled_fwd<maxpool3d_tiled_fwd_kernel<KT, KH, KW, ST, SH, SW, WPT, false>>,
           &launch_tiled_fwd<maxpool3d_tiled_fwd_kernel<KT, KH, KW, ST, SH, SW, WPT, true>>}};
}
// the row number is out[1] of coclr_pool_plan (ops.PoolGeom._FWD_TILED mirrors the rows in this order)
constexpr TiledFwdRow kTiledFwd[] = {
    tiled_fwd_row<1, 3, 3, 1, 2, 2, 2>(), tiled_fwd_row<3, 3, 3, 1, 1, 1, 4>(),
    tiled_fwd_row<3, 3, 3, 2, 2, 2, 2>(), tiled_fwd_row<2, 2, 2, 2, 2, 2, 2>()};
constexpr int kTiledFwdRows = sizeof(kTiledFwd) / sizeof(kTiledFwd[0]);
constexpr bool tiled_fwd_is(const TiledFwdRow& r, int kt, int kh, int kw, int st, int sh, int sw, int wpt = 0) {
  return r.kt == kt && r.kh == kh && r.kw == kw && r.st == st && r.sh == sh && r.sw == sw && (!wpt || r.wpt == wpt);
}
static_assert(kTiledFwdRows == 4 && tiled_fwd_is(kTiledFwd[0], 1, 3, 3, 1, 2, 2, 2) &&
              tiled_fwd_is(kTiledFwd[1], 3, 3, 3, 1, 1, 1, 4) && tiled_fwd_is(kTiledFwd[2], 3, 3, 3, 2, 2, 2, 2) &&
              tiled_fwd_is(kTiledFwd[3], 2, 2, 2, 2, 2, 2, 2), "row order is the out[1] contract of coclr_pool_plan");

// separable 3x3x3: TT frames at compile time; the last row (TT = 0) takes the frame count at run time
struct Sep333Row { int tt; PoolFwdFn launch[2]; };
template <int TT>
constexpr Sep333Row sep333_row() {
  return {TT, {&launch_sep333<maxpool333_kernel<false, TT>>, &launch_sep333<maxpool333_kernel<true, TT>>}};
}
constexpr Sep333Row kSep333[] = {sep333_row<16>(), sep333_row<8>(), sep333_row<4>(), sep333_row<0>()};
constexpr int kSep333Rows = sizeof(kSep333) / sizeof(kSep333[0]);
static_assert(kSep333[kSep333Rows - 1].tt == 0, "the run-time frame count form is the fallback");
inline PoolFwdPlan plan_pool_fwd(const PoolGeom& g, bool with_idx) {
  PoolFwdPlan p;
  p.family = kFwdGeneric; p.tmpl = 0; p.G = 1; p.tfold = 1; p.vec = 0; p.lds = 0; p.lW = p.lHW = 0;
  p.planes = g.N * g.C;
  p.g = g;
  p.launch = nullptr;
  if (is_333_s1_p1(g)) {
    // inception pool branch: separable scan, thread = (volume, h, w)
    const int lW = ilog2_exact(g.Wi), lHW = ilog2_exact(g.Hi * g.Wi);
    if (lW >= 0 && lHW >= 4 && lHW <= 8 && g.Ti <= 32) {
      const int PG = 256 >> lHW, S = g.Ti << lHW;
      const size_t lds = (size_t)PG * S * 4 * (with_idx ? 3 : 2);
      if (lds <= 64 * 1024) {
        const Sep333Row* row = &kSep333[kSep333Rows - 1];
        for (const Sep333Row& r : kSep333)
          if (r.tt == g.Ti) { row = &r; break; }
        p.family = kFwdSep333; p.tmpl = row->tt; p.launch = row->launch;
        p.G = PG; p.gx = cdiv(p.planes, PG); p.gy = 1;
        p.vec = (g.x_nstride & 3) == 0;
        p.lds = (int)lds; p.lW = lW; p.lHW = lHW;
        return p;
      }
    }
  }
  {
    // LDS-tiled fast paths; T is folded into the plane count when the stencil ignores it
    const PoolGeom f = fold_time(g);
    const int Si = f.Ti * f.Hi * f.Wi;
    const int planes = f.N * f.C;
    if (Si <= kTileFloats) {
      for (int row = 0; row < kTiledFwdRows; ++row) {
        if (!tiled_fwd_is(kTiledFwd[row], f.kt, f.kh, f.kw, f.st, f.sh, f.sw)) continue;
        // ~16 KiB tiles: 8 workgroups per CU so the load, scan and store phases of different
        // workgroups overlap (64 KiB tiles left 2 per CU and ran at 1.2 TB/s)
        const int G = volumes_per_wg(planes, Si, 4096, 2048);
        p.family = kFwdTiled; p.tmpl = row; p.launch = kTiledFwd[row].launch;
        p.G = G; p.gx = (planes + G - 1) / G; p.gy = 1;
        p.tfold = f.Ti == g.Ti ? 1 : g.Ti;
        p.vec = (Si & 3) == 0 && (f.x_nstride & 3) == 0;
        p.lds = (int)((size_t)G * Si * sizeof(float));
        p.planes = planes;
        p.g = f;
        return p;
      }
    }
  }
  const dim3 grid = pool_grid(g.N * g.C, g.To * g.Ho * g.Wo);
  p.gx = (int)grid.x; p.gy = (int)grid.y;
  return p;
}

// ---- backward ---------------------------------------------------------------------------------------------------
// colour-class counts of a pool and the outputs a thread holds per class for G volumes per workgroup
struct ClassShape { int pt, ph, pw, kq; };
inline ClassShape class_shape(const PoolGeom& g, int G) {
  ClassShape c;
  c.pt = (g.kt + g.st - 1) / g.st; c.ph = (g.kh + g.sh - 1) / g.sh; c.pw = (g.kw + g.sw - 1) / g.sw;
  const long m = (long)((g.To + c.pt - 1) / c.pt) * ((g.Ho + c.ph - 1) / c.ph) * ((g.Wo + c.pw - 1) / c.pw);
  c.kq = (int)((G * m + 255) / 256);
  static const bool off = getenv("COCLR_POOL_PRELOAD") && atoi(getenv("COCLR_POOL_PRELOAD")) == 0;
  if (off) c.kq = 1 << 20;            // A/B switch: the generic one-round-trip-per-class form
  return c;
}

// A colour-class template: PT, PH, PW, KQ and the function that launches that instantiation.  A pool takes the
// first row of its table with its class counts and kq <= KQ, else the table's generic <0, 0, 0, 0> row.
template <typename Fn>
struct ClassRow { int pt, ph, pw, kq; Fn launch; };

template <typename Fn, int NR>
const ClassRow<Fn>* pick_class_template(const ClassShape& cs, const ClassRow<Fn> (&rows)[NR],
                                        const ClassRow<Fn>* generic) {
  for (const ClassRow<Fn>& r : rows)
    if (cs.pt == r.pt && cs.ph == r.ph && cs.pw == r.pw && cs.kq <= r.kq) return &r;
  return generic;
}
// first match wins: a later row with the same class counts must have the larger KQ (no duplicate, none unreachable)
template <typename Fn, int NR>
constexpr bool class_rows_ordered(const ClassRow<Fn> (&r)[NR]) {
  for (int i = 0; i < NR; ++i)
    for (int j = i + 1; j < NR; ++j)
      if (r[i].pt == r[j].pt && r[i].ph == r[j].ph && r[i].pw == r[j].pw && r[i].kq >= r[j].kq) return false;
  return true;
}

struct PoolBwdPlan;
typedef int (*PoolBwdFn)(const PoolBwdPlan&, const float* dy, const int32_t* idx, float* dx, long dy_nstride,
                         long dx_nstride, int accumulate, hipStream_t);

struct PoolBwdPlan {
  int family;        // kBwd*
  const ClassRow<PoolBwdFn>* row;   // colour classes: the template row (kBwdGenericRow: generic form), else nullptr
  int G, kq;         // volumes per workgroup; outputs per thread and class for that G (colour classes)
  int gx, gy;
  int tfold;
  int vec;           // 333 gather: 16-byte staging of dy / indices; colour classes: 16-byte stores of dx
  int lds;
  int lW, lHW;       // 333 gather only
  int planes, Si;
  PoolGeom g;
};

template <int PT, int PH, int PW, int KQ>
int launch_tiled_bwd(const PoolBwdPlan& p, const float* dy, const int32_t* idx, float* dx, long dy_nstride,
                     long dx_nstride, int accumulate, hipStream_t st) {
  return launch_dyn_lds<maxpool3d_tiled_bwd_kernel<PT, PH, PW, KQ>, 256, kTileFloats * 4>(
      dim3(p.gx), (size_t)p.lds, st, dy, idx, dx, p.g, dy_nstride, dx_nstride, accumulate, p.G, p.planes, p.tfold,
      p.vec);
}
template <int PT, int PH, int PW, int KQ>
constexpr ClassRow<PoolBwdFn> bwd_row() { return {PT, PH, PW, KQ, &launch_tiled_bwd<PT, PH, PW, KQ>}; }

constexpr ClassRow<PoolBwdFn> kBwdTemplates[] = {bwd_row<1, 2, 2, 1>(), bwd_row<3, 3, 3, 1>(), bwd_row<2, 2, 2, 1>(),
                                                 bwd_row<1, 1, 1, 2>()};
constexpr ClassRow<PoolBwdFn> kBwdGenericRow = bwd_row<0, 0, 0, 0>();
inline PoolBwdPlan plan_pool_bwd(const PoolGeom& g0, long dy_nstride, long dx_nstride) {
  PoolBwdPlan p;
  p.family = kBwdGeneric; p.row = nullptr; p.G = 1; p.kq = 0; p.tfold = 1; p.vec = 0; p.lds = 0; p.lW = p.lHW = 0;
  p.planes = g0.N * g0.C; p.Si = g0.Ti * g0.Hi * g0.Wi;
  p.g = g0;
  if (is_333_s1_p1(g0)) {
    const int lW = ilog2_exact(g0.Wi), lHW = ilog2_exact(g0.Hi * g0.Wi);
    const int S = p.Si;
    // measured (B=32): 4x4x4 volumes 0.027 ms gather vs 0.055 colour classes; 8x8x8 0.084 vs 0.075;
    // 16x16x16 0.327 vs 0.158 -- the 27-candidate scan is VALU-bound, it only pays on tiny volumes
    if (lW >= 0 && lHW >= 0 && S <= 128) {
      const int G = volumes_per_wg(p.planes, S, 2048, 2048);   // ~16 KiB of LDS (dy + indices): 8 workgroups per CU
      p.family = kBwdGather333; p.G = G; p.gx = (p.planes + G - 1) / G; p.gy = 1;
      p.vec = (S & 3) == 0 && (dy_nstride & 3) == 0;
      p.lds = G * S * 8; p.lW = lW; p.lHW = lHW;
      return p;
    }
  }
  {
    const PoolGeom g = fold_time(g0);
    const int Si = g.Ti * g.Hi * g.Wi;
    const int planes = g.N * g.C;
    if (Si <= kTileFloats) {
      // a colour class holds ~1/27 of a volume's outputs: keep enough volumes per workgroup for its
      // 256 threads (1024 workgroups still fill the chip four deep)
      const int G = volumes_per_wg(planes, Si, 4096, 1024);
      const ClassShape cs = class_shape(g, G);
      p.family = kBwdClasses; p.row = pick_class_template(cs, kBwdTemplates, &kBwdGenericRow);
      p.G = G; p.kq = cs.kq; p.gx = (planes + G - 1) / G; p.gy = 1;
      p.tfold = g.Ti == g0.Ti ? 1 : g0.Ti;
      p.vec = (Si & 3) == 0 && (dx_nstride & 3) == 0;
      p.lds = (int)((size_t)G * Si * sizeof(float));
      p.planes = planes; p.Si = Si;
      p.g = g;
      return p;
    }
  }
  const dim3 grid = pool_grid(g0.N * g0.C, g0.Ti * g0.Hi * g0.Wi);
  p.gx = (int)grid.x; p.gy = (int)grid.y;
  return p;
}

// ---- BatchNorm backward behind a pool ---------------------------------------------------------------------------
struct PooledBnPlan;
struct PooledBnOperands {
  const float* pool_dy; const int32_t* pool_idx;
  const float* y; const float* scale; const float* shift; const float* mean; const float* invstd;
  double* sums;
  float* dy; float* dgamma; float* dbeta;
  long pool_dy_nstride, y_nstride, dy_nstride;
  int relu, training;
};
typedef int (*PooledBnFn)(const PooledBnPlan&, const PooledBnOperands&, hipStream_t);

struct PooledBnPlan {
  int fits;
  const ClassRow<PooledBnFn>* row;   // the template row (kPooledGenericRow: generic form); nullptr when !fits
  int G, kq, blocks, tfold, vec, lds, planes, Si;
  PoolGeom g;
};

template <int PT, int PH, int PW, int KQ>
int launch_pooled_bn(const PooledBnPlan& p, const PooledBnOperands& a, hipStream_t st) {
  const double count = (double)p.g.N * (p.Si * p.tfold);        // elements per channel of the unfolded geometry
  return launch_dyn_lds<bn_pool_bwd_apply_kernel<PT, PH, PW, KQ>, 256, kTileFloats * 4>(
      dim3(p.blocks), (size_t)p.lds, st, a.pool_dy, a.pool_idx, a.y, a.scale, a.shift, a.mean, a.invstd, a.sums,
      p.g.N, count, a.training, a.dgamma, a.dbeta, a.dy, p.g, a.pool_dy_nstride, a.y_nstride, a.dy_nstride, a.relu,
      p.G, p.planes, p.tfold, p.vec);
}
template <int PT, int PH, int PW, int KQ>
constexpr ClassRow<PooledBnFn> pooled_row() { return {PT, PH, PW, KQ, &launch_pooled_bn<PT, PH, PW, KQ>}; }

constexpr ClassRow<PooledBnFn> kPooledTemplates[] = {pooled_row<1, 2, 2, 1>(), pooled_row<2, 2, 2, 1>()};
constexpr ClassRow<PooledBnFn> kPooledGenericRow = pooled_row<0, 0, 0, 0>();
static_assert(class_rows_ordered(kBwdTemplates) && class_rows_ordered(kPooledTemplates), "duplicate / unreachable row");

inline PooledBnPlan plan_pooled_bn(const PoolGeom& g0, long y_nstride, long dy_nstride) {
  PooledBnPlan p;
  const PoolGeom g = fold_time(g0);
  p.g = g;
  p.tfold = g.Ti == g0.Ti ? 1 : g0.Ti;
  p.Si = g.Ti * g.Hi * g.Wi;
  p.planes = g.N * g.C;
  p.fits = p.Si <= kTileFloats;
  p.row = nullptr; p.G = 0; p.kq = 0; p.blocks = 0; p.vec = 0; p.lds = 0;
  if (!p.fits) return p;
  const int G = volumes_per_wg(p.planes, p.Si, 4096, 1024, 8);   // at most 8: coef[8][4] of the apply kernel
  const ClassShape cs = class_shape(g, G);
  p.row = pick_class_template(cs, kPooledTemplates, &kPooledGenericRow);
  p.G = G; p.kq = cs.kq; p.blocks = (p.planes + G - 1) / G;
  p.vec = (p.Si & 3) == 0 && ((y_nstride | dy_nstride) & 3) == 0;
  p.lds = (int)((size_t)G * p.Si * sizeof(float));
  return p;
}

}  // namespace

extern "C" int coclr_maxpool3d_fwd(const coclr_pool_desc* d, const float* x, float* y,
                                   int32_t* indices, const float* in_scale, const float* in_shift,
                                   int in_relu, void* stream) {
  if (!d || d->N <= 0 || d->C <= 0) return COCLR_EINVAL;
  if (d->pt * 2 > d->kt || d->ph * 2 > d->kh || d->pw * 2 > d->kw) return COCLR_EINVAL;
  if ((in_scale == nullptr) != (in_shift == nullptr)) return COCLR_EINVAL;
  PoolGeom g = to_geom(d);
  g.in_scale = in_scale; g.in_shift = in_shift; g.in_relu = in_relu;
  const PoolFwdPlan p = plan_pool_fwd(g, indices != nullptr);
  hipStream_t st = (hipStream_t)stream;
  if (p.launch) return p.launch[indices != nullptr](p, x, y, indices, st);
  hipLaunchKernelGGL(maxpool3d_fwd_kernel, dim3(p.gx, p.gy), dim3(256), 0, st, x, y, indices, g);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_maxpool3d_bwd(const coclr_pool_desc* d, const float* dy, const int32_t* indices,
                                   float* dx, int64_t dy_nstride, int64_t dx_nstride,
                                   int accumulate, void* stream) {
  if (!d || d->N <= 0 || d->C <= 0) return COCLR_EINVAL;
  const PoolGeom g0 = to_geom(d);
  const PoolBwdPlan p = plan_pool_bwd(g0, (long)dy_nstride, (long)dx_nstride);
  hipStream_t st = (hipStream_t)stream;
  if (p.row) return p.row->launch(p, dy, indices, dx, (long)dy_nstride, (long)dx_nstride, accumulate, st);
  if (p.family == kBwdGather333)
    hipLaunchKernelGGL(maxpool333_bwd_kernel, dim3(p.gx), dim3(256), (size_t)p.lds, st, dy, indices, dx, g0,
                       (long)dy_nstride, (long)dx_nstride, accumulate, p.G, p.planes, p.lW, p.lHW, p.vec);
  else
    hipLaunchKernelGGL(maxpool3d_bwd_kernel, dim3(p.gx, p.gy), dim3(256), 0, st, dy, indices, dx, g0,
                       (long)dy_nstride, (long)dx_nstride, accumulate);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_bn_act_backward_pooled_fits(const coclr_pool_desc* d, int* fits) {
  if (!d || !fits || d->N <= 0 || d->C <= 0) return COCLR_EINVAL;
  *fits = plan_pooled_bn(to_geom(d), 0, 0).fits;
  return 0;
}

extern "C" int coclr_bn_act_backward_pooled(const coclr_pool_desc* d, const float* pool_dy,
                                            const int32_t* pool_idx, const float* y,
                                            const float* scale, const float* shift,
                                            const float* mean, const float* invstd, double* sums,
                                            float* dy, float* dgamma, float* dbeta,
                                            int64_t pool_dy_nstride, int64_t y_nstride,
                                            int64_t dy_nstride, int relu, int training, void* stream) {
  if (!d || d->N <= 0 || d->C <= 0 || !pool_dy || !pool_idx || !y || !sums || !dy) return COCLR_EINVAL;
  const PoolGeom g0 = to_geom(d);
  const PooledBnPlan p = plan_pooled_bn(g0, (long)y_nstride, (long)dy_nstride);
  if (!p.fits) return COCLR_EINVAL;                   // see coclr_bn_act_backward_pooled_fits
  hipStream_t st = (hipStream_t)stream;
  const int So0 = g0.To * g0.Ho * g0.Wo, Si0 = g0.Ti * g0.Hi * g0.Wi;
  hipLaunchKernelGGL(bn_pool_bwd_reduce_kernel, dim3(g0.C, g0.N), dim3(256), 0, st, pool_dy, pool_idx,
                     y, scale, shift, mean, invstd, sums, g0.C, So0, Si0, (long)pool_dy_nstride,
                     (long)y_nstride, relu);
  COCLR_LAUNCH_CHECK();
  const PooledBnOperands a = {pool_dy, pool_idx, y, scale, shift, mean, invstd, sums, dy, dgamma, dbeta,
                              (long)pool_dy_nstride, (long)y_nstride, (long)dy_nstride, relu, training};
  return p.row->launch(p, a, st);
}

// What the three launchers above would do for this descriptor, nothing launched (usable without a device).
// dy_nstride / dx_nstride: sample strides of the backward's operands, 0: dense.  The pooled BatchNorm backward is
// planned with y at the descriptor's x_nstride and its dy at dx_nstride (they have x's and dx's layout).
extern "C" int coclr_pool_plan(const coclr_pool_desc* d, int with_indices, int64_t dy_nstride,
                               int64_t dx_nstride, int32_t out[32]) {
  if (!d || !out || d->N <= 0 || d->C <= 0) return COCLR_EINVAL;
  if (d->pt * 2 > d->kt || d->ph * 2 > d->kh || d->pw * 2 > d->kw) return COCLR_EINVAL;
  const PoolGeom g = to_geom(d);
  if (!dy_nstride) dy_nstride = (int64_t)d->C * d->To * d->Ho * d->Wo;
  if (!dx_nstride) dx_nstride = (int64_t)d->C * d->Ti * d->Hi * d->Wi;
  for (int i = 0; i < 32; ++i) out[i] = 0;
  const PoolFwdPlan f = plan_pool_fwd(g, with_indices != 0);
  out[0] = f.family; out[1] = f.tmpl; out[2] = f.G; out[3] = f.gx; out[4] = f.gy; out[5] = f.tfold;
  out[6] = f.vec; out[7] = f.lds;
  const PoolBwdPlan b = plan_pool_bwd(g, (long)dy_nstride, (long)dx_nstride);
  out[8] = b.family;
  if (b.row) { out[9] = b.row->pt; out[10] = b.row->ph; out[11] = b.row->pw; out[12] = b.row->kq; }
  out[13] = b.G; out[14] = b.kq; out[15] = b.gx; out[16] = b.gy; out[17] = b.tfold; out[18] = b.vec; out[19] = b.lds;
  const PooledBnPlan q = plan_pooled_bn(g, (long)d->x_nstride, (long)dx_nstride);
  out[20] = q.fits; out[21] = q.G;
  if (q.row) { out[22] = q.row->pt; out[23] = q.row->ph; out[24] = q.row->pw; out[25] = q.row->kq; }
  out[26] = q.kq; out[27] = q.blocks; out[28] = q.tfold; out[29] = q.vec; out[30] = q.lds;
  out[31] = g.nt;
  return 0;
}

extern "C" int coclr_global_avgpool_fwd(const float* x, float* y, int64_t planes, int64_t S,
                                        void* stream) {
  if (planes <= 0 || S <= 0) return COCLR_EINVAL;
  hipLaunchKernelGGL(global_avgpool_fwd_kernel, dim3(cdiv(planes * 64, 256)), dim3(256), 0,
                     (hipStream_t)stream, x, y, (int)planes, (int)S);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_global_avgpool_bwd(const float* dy, float* dx, int64_t planes, int64_t S,
                                        void* stream) {
  if (planes <= 0 || S <= 0) return COCLR_EINVAL;
  const long total = planes * S;
  int blocks = cdiv(total, 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(global_avgpool_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy,
                     dx, total, (int)S);
  COCLR_LAUNCH_CHECK();
  return 0;
}
