// Baseline JPEG frames -> uint8 (F, H, W, 3) on the device, bit-identical to libjpeg-turbo's default decoder
// (what PIL's Image.open(...).convert('RGB') returns; dataset/lmdb_dataset.py:37-38 of the reference).
// Three stages, one kernel each; the arithmetic lives in jpeg_core.h, shared with a host build:
//   1 entropy   one lane per (frame, restart segment): Huffman -> dequantised int16 coefficients
//   2 idct      one lane per 8x8 block: coefficients -> sample planes at the component's own resolution
//   4 colour    one lane per 16 output pixels of a row: chroma upsampling, YCbCr -> RGB, crop to (H, W)
// Huffman decoding is serial inside a restart segment, so a frame without restart markers is ONE lane of stage 1.
#include "../../include/coclr_hip.h"
#include "common.h"
#include "jpeg_core.h"

namespace {

constexpr int JPEG_MAX_SIDE = 8192;

// one wave per workgroup: with one lane per frame, 64 frames are all a CU gets, so the waves spread over the CUs
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ data, int data_len,
                                                          const int32_t* __restrict__ meta, int width, int F,
                                                          int maxseg, jc_geom g, int16_t* __restrict__ coef,
                                                          int32_t* __restrict__ status) {
  const long id = (long)blockIdx.x * 64 + threadIdx.x;
  const long f = id / maxseg;
  const int seg = (int)(id % maxseg);
  if (f >= F) return;
  const int32_t* m = meta + f * width;
  int s0, s1, m0, m1;
  if (!jc_segment_range(m, width, maxseg, data_len, seg, g, &s0, &s1, &m0, &m1)) return;
  const int st = jc_decode_segment(data, s0, s1, m, g, m0, m1, coef + f * (long)g.nblocks * 64);
  if (st) atomicOr(&status[f], st);
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, long n, jc_geom g,
                                                        uint8_t* __restrict__ planes) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const long f = id / g.nblocks;
  const int blk = (int)(id % g.nblocks);
  __attribute__((aligned(16))) int16_t in[64];
  const uint4* src = reinterpret_cast<const uint4*>(coef + id * 64);      // 128 bytes per block, 16-byte aligned
#pragma unroll
  for (int i = 0; i < 8; ++i) reinterpret_cast<uint4*>(in)[i] = src[i];
  long stride;
  const long at = jc_block_samples(g, blk, &stride);
  jc_idct_block(in, planes + f * (long)g.nblocks * 64 + at, stride);
}

// vec: W % 16 == 0 and `out` 16-byte aligned, so every group of 16 pixels is three aligned 16-byte stores
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, long n, int groups,
                                                          jc_geom g, int vec, uint8_t* __restrict__ out) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const int xg = (int)(id % groups);
  const long row = id / groups;
  const int y = (int)(row % g.H);
  const long f = row / g.H;
  const uint8_t* p = planes + f * (long)g.nblocks * 64;
  uint8_t* o = out + (row * g.W + (long)xg * 16) * 3;
  const int x0 = xg * 16;
  if (vec) {
    __attribute__((aligned(16))) uint8_t px[48];
#pragma unroll
    for (int i = 0; i < 16; ++i) jc_pixel(p, g, x0 + i, y, px + 3 * i);
#pragma unroll
    for (int i = 0; i < 3; ++i) reinterpret_cast<uint4*>(o)[i] = reinterpret_cast<const uint4*>(px)[i];
  } else {
    const int nx = g.W - x0 < 16 ? g.W - x0 : 16;
    for (int i = 0; i < nx; ++i) {
      uint8_t px[3];
      jc_pixel(p, g, x0 + i, y, px);
      o[3 * i] = px[0];
      o[3 * i + 1] = px[1];
      o[3 * i + 2] = px[2];
    }
  }
}

bool geometry_ok(int H, int W, int ncomp, int hs, int vs) {
  if (H < 1 || W < 1 || H > JPEG_MAX_SIDE || W > JPEG_MAX_SIDE) return false;
  if (ncomp == 1) return hs == 1 && vs == 1;
  return ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}

// what the kernels rely on, checked on the host copy of the descriptors
bool meta_ok(const int32_t* meta, int F, int width, int64_t data_len, const jc_geom& g, int* maxseg) {
  const long total = (long)g.mcux * g.mcuy;
  int most = 1;
  for (int f = 0; f < F; ++f) {
    const int32_t* m = meta + (long)f * width;
    const long off = m[JM_OFF], len = m[JM_LEN], ri = m[JM_RI], nseg = m[JM_NSEG];
    if (off < 0 || len < 0 || off + len > data_len) return false;
    if (ri < 0 || nseg < 1 || nseg > width - JM_SEG) return false;
    if (nseg != (ri == 0 ? 1 : (total + ri - 1) / ri)) return false;
    long last = 0;
    for (int s = 0; s < nseg; ++s) {
      const long at = m[JM_SEG + s];
      if (at < last || at > len) return false;
      last = at;
    }
    for (int i = 0; i < 64 * g.ncomp; ++i)
      if (m[JM_QUANT + i] < 0 || m[JM_QUANT + i] > 255) return false;
    for (int t = 0; t < 6; ++t) {
      const int32_t* h = m + JM_HUFF + t * JM_HUFF_WORDS;
      for (int l = 0; l < 16; ++l)
        if (h[l] < 0 || h[l] > 65536 || (l && h[l] < h[l - 1]) || h[16 + l] < -65536 || h[16 + l] > 255) return false;
    }
    if (nseg > most) most = (int)nseg;
  }
  *maxseg = most;
  return true;
}

}  // namespace

extern "C" int coclr_jpeg_workspace(int H, int W, int ncomp, int hs, int vs, int64_t* coef_bytes,
                                    int64_t* plane_bytes) {
  if (!coef_bytes || !plane_bytes || !geometry_ok(H, W, ncomp, hs, vs)) return COCLR_EINVAL;
  jc_geom g;
  jc_geom_init(g, H, W, ncomp, hs, vs);
  *coef_bytes = (int64_t)g.nblocks * 128;
  *plane_bytes = (int64_t)g.nblocks * 64;
  return 0;
}

extern "C" int coclr_jpeg_decode(const uint8_t* data, int64_t data_len, const int32_t* meta, const int32_t* meta_host,
                                 int F, int width, int H, int W, int ncomp, int hs, int vs, int stages, int16_t* coefs,
                                 uint8_t* planes, uint8_t* out, int32_t* status, void* stream) {
  if (!data || !meta || !meta_host || !coefs || !planes || !out || !status) return COCLR_EINVAL;
  if (F < 1 || width <= JM_SEG || data_len < 0 || data_len > 0x7fffffff || stages < 1 || stages > 7)
    return COCLR_EINVAL;
  if (!geometry_ok(H, W, ncomp, hs, vs) || ((uintptr_t)coefs & 15) || ((uintptr_t)meta & 3)) return COCLR_EINVAL;
  jc_geom g;
  jc_geom_init(g, H, W, ncomp, hs, vs);
  int maxseg = 1;
  if (!meta_ok(meta_host, F, width, data_len, g, &maxseg)) return COCLR_EINVAL;
  const int groups = (W + 15) / 16;
  const long lanes1 = (long)F * maxseg, lanes2 = (long)F * g.nblocks, lanes3 = (long)F * H * groups;
  const long limit = 0x7fffffffL;        // workgroups of one launch
  if (lanes1 / 64 >= limit || lanes2 / 256 >= limit || lanes3 / 256 >= limit) return COCLR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (stages & 1) {
    COCLR_RETURN_IF(hipMemsetAsync(coefs, 0, (size_t)F * g.nblocks * 128, s));
    COCLR_RETURN_IF(hipMemsetAsync(status, 0, (size_t)F * 4, s));
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(cdiv(lanes1, 64)), dim3(64), 0, s, data, (int)data_len, meta, width,
                       F, maxseg, g, coefs, status);
    COCLR_LAUNCH_CHECK();
  }
  if (stages & 2) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(cdiv(lanes2, 256)), dim3(256), 0, s, coefs, lanes2, g, planes);
    COCLR_LAUNCH_CHECK();
  }
  if (stages & 4) {
    const int vec = W % 16 == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(cdiv(lanes3, 256)), dim3(256), 0, s, planes, lanes3, groups, g, vec,
                       out);
    COCLR_LAUNCH_CHECK();
  }
  return 0;
}
