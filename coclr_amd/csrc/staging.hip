// Input staging of the training loop for gfx950 (main_nce.py:207-209,299-302,310;
// main_coclr.py:221-223,366-368; utils/transforms.py:57-63; model/pretrain.py:149-150).
//
// The reference receives fp32 frames (B, 3, num_seq*seq_len, H, W) in [0,1] from the loader
// (403 MB/step over PCIe at B=32), normalises them on the GPU (one full-tensor pass), then
// .view().transpose(1,2).contiguous() (a second full copy) and the model .contiguous()-copies each
// clip again.  Here the loader's frames may stay uint8 (101 MB/step over PCIe) and ONE kernel does
// ToTensor's /255, Normalize(mean, std, channel=1) and the (B,C,S,T,H,W) -> (B,S,C,T,H,W)
// re-layout: 1 (or 4) bytes read + 4 bytes written per element, 16-byte accesses.  Arithmetic is
// the reference's, operation for operation (x/255, then (x-mean)/std with IEEE division), so the
// result is bit-identical to ToTensor + Normalize on the same bytes.
#include "common.h"
#include "../../include/coclr_hip.h"

#pragma clang fp contract(off)      // bit-identical to ToTensor + Normalize: every operation rounded

namespace {

struct StageArgs {
  const void* in; float* out;
  float mean[4], std[4];
  int C, S;
  long THW;        // elements of one (b, c, s) run: seq_len*H*W, contiguous on both sides
  int from_u8;
  int vec;         // StagePlan::vec: 16-byte loads and stores, every run of `in` AND of `out` starts 16-byte aligned
};

__device__ __forceinline__ float norm1(float x, float mean, float std) {
  return __fdiv_rn(__fsub_rn(x, mean), std);
}

template <bool U8>
__global__ void __launch_bounds__(256)
stage_clips_kernel(const StageArgs a) {
  // blockIdx.y = (b*C + c)*S + s on the source side
  const int run = blockIdx.y;
  const int s = run % a.S, bc = run / a.S;
  const int c = bc % a.C, b = bc / a.C;
  const float mean = a.mean[c], std = a.std[c];
  float* dst = a.out + (((long)b * a.S + s) * a.C + c) * a.THW;
  if (U8) {
    const uint8_t* src = static_cast<const uint8_t*>(a.in) + (long)run * a.THW;
    if (a.vec) {
      const long n16 = a.THW >> 4;
      for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) {
        const uint4 q = reinterpret_cast<const uint4*>(src)[i];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float4 o;
          o.x = norm1(__fdiv_rn((float)(w[k] & 255u), 255.f), mean, std);
          o.y = norm1(__fdiv_rn((float)((w[k] >> 8) & 255u), 255.f), mean, std);
          o.z = norm1(__fdiv_rn((float)((w[k] >> 16) & 255u), 255.f), mean, std);
          o.w = norm1(__fdiv_rn((float)(w[k] >> 24), 255.f), mean, std);
          reinterpret_cast<float4*>(dst)[i * 4 + k] = o;
        }
      }
    } else {
      for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.THW; i += (long)gridDim.x * 256)
        dst[i] = norm1(__fdiv_rn((float)src[i], 255.f), mean, std);
    }
  } else {
    const float* src = static_cast<const float*>(a.in) + (long)run * a.THW;
    if (a.vec) {
      const long n4 = a.THW >> 2;
      for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 q = reinterpret_cast<const float4*>(src)[i];
        float4 o;
        o.x = norm1(q.x, mean, std); o.y = norm1(q.y, mean, std);
        o.z = norm1(q.z, mean, std); o.w = norm1(q.w, mean, std);
        reinterpret_cast<float4*>(dst)[i] = o;
      }
    } else {
      for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.THW; i += (long)gridDim.x * 256)
        dst[i] = norm1(src[i], mean, std);
    }
  }
}

// ---- five/ten-crop test clips from raw frames (eval/main_classifier.py:453-469; utils/augmentation.py:21-43,
// 61-88,149-177,347-350) -----------------------------------------------------------------------------------
// flip -> FiveCrop -> Scale(BICUBIC) -> ToTensor -> Normalize -> (crop, clip, 3, T, S, S), one launch per video.
// Scale is PIL's Image.resize on 8-bit pixels: separable, horizontal pass first, 22-bit fixed-point
// coefficients, (2^21 + sum K*src) >> 22 clamped to uint8 after EACH pass -- integer arithmetic, so the result is
// PIL's bit for bit given PIL's coefficient tables (built on the host in double: coclr_amd/staging.py).
// One workgroup per (band of R output rows, slot = (clip, t), crop): the horizontal pass of the band's source
// rows goes to LDS as uint8 [row][c][Sp], four results per lane and one 4-byte LDS store; after the barrier the
// vertical pass reads one 4-byte LDS word per tap, converts with the arithmetic of stage_clips_kernel above and
// stores 16 bytes along x.  A flipped crop reads source column W-1-(x0+j) with the SAME tables.
// Every table-derived index is clamped (v_med3) into the crop box / the staged rows: the tables are device
// data, and zero-padded taps point past the box.
struct CropArgs {
  const uint8_t* frames; const int32_t* slot_frame;
  const int32_t *xmin, *xk, *ymin, *yk;      // [Sp], [taps][Sp]
  float* out;                                // fp32 form: [crop][clip][3][T][S][S], normalised
  uint8_t* out8;                             // uint8 form: [crop][clip*T][S][S][3], the resized bytes themselves
  int crop[16][3];                           // x0, y0, flip
  float mean[3], std[3];
  int F, H, W, T, n_clips, cw, ch, S, Sp, xtaps, ytaps, R, cap_rows;
  // the ragged form (coclr_stage_crops_ragged): one descriptor per output clip, one byte offset per slot
  const int32_t* desc; const int64_t* slot_off;
  long nbytes;                               // bytes of `frames`
};

// The RAGGED form of the crop kernel: the clips of MANY videos, of differing frame sizes, in one launch.  An output
// clip is one (video, crop, clip) triple with its own descriptor {x0, y0, flip, W, H} (device data, int32 x
// CROP_FIELDS); `frames` is one flat byte buffer and slot_off[clip*T + t] the byte offset of the frame that slot
// reads (64 bits; test clips are strided, padded and overlapping, so there is no step from one slot to the next).
// The crop SIZE and the tables stay those of the launch.  W, H and the box are clamped to the clip's OWN frame, and a
// slot whose frame would not lie inside the buffer of `nbytes`, or is smaller than the crop, is skipped, so nothing
// is read outside it whatever the device copies hold (the entry point validates the host copies before the launch).
enum { CROP_X0 = 0, CROP_Y0, CROP_FLIP, CROP_W, CROP_H, CROP_FIELDS };
constexpr int kRagMaxSide = 32768;

struct CropRows { const uint8_t* fr; int x0, flip, W; };     // fr: row y0 + ylo of the frame, column 0

template <bool RAGGED>
__device__ __forceinline__ bool crop_rows(const CropArgs& a, int slot, int crop, int ylo, CropRows& o) {
  if (RAGGED) {
    const int32_t* d = a.desc + (long)(slot / a.T) * CROP_FIELDS;
    const int W = min(max(d[CROP_W], 1), kRagMaxSide), H = min(max(d[CROP_H], 1), kRagMaxSide);
    const long off = a.slot_off[slot];
    if (W < a.cw || H < a.ch || off < 0 || off > a.nbytes - (long)W * H * 3) return false;
    const int y0 = min(max(d[CROP_Y0], 0), H - a.ch);
    o.x0 = min(max(d[CROP_X0], 0), W - a.cw);
    o.flip = d[CROP_FLIP] != 0;
    o.W = W;
    o.fr = a.frames + off + (long)(y0 + ylo) * W * 3;
  } else {
    const int y0 = a.crop[crop][1];
    const int f = min(max(a.slot_frame[slot], 0), a.F - 1);
    o.x0 = a.crop[crop][0];
    o.flip = a.crop[crop][2];
    o.W = a.W;
    o.fr = a.frames + ((long)f * a.H + (y0 + ylo)) * (long)a.W * 3;
  }
  return true;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ unsigned fix8(int acc) {       // PIL's clip8 of a 22-bit fixed-point sum
  const int t = max(acc + (1 << 21), 0);                  // negative sums clip to 0, so the shift can be logical
  return min((unsigned)t >> 22, 255u);
}

template <bool U8OUT, bool RAGGED>
__global__ void __launch_bounds__(256)
stage_crops_kernel(const CropArgs a) {
  extern __shared__ __align__(16) uint8_t hrows[];      // [rows][3][Sp]
  const int tid = threadIdx.x;
  const int band = blockIdx.x, slot = blockIdx.y, crop = RAGGED ? 0 : blockIdx.z;
  const int r0 = band * a.R, r1 = min(r0 + a.R, a.S);                  // output rows [r0, r1)
  const int ylo = clampi(a.ymin[r0], 0, a.ch - 1);
  const int rows = min(clampi(a.ymin[r1 - 1] + a.ytaps, ylo + 1, a.ch) - ylo, a.cap_rows);
  const int Sp = a.Sp, nxg = Sp >> 2;
  CropRows g;
  if (!crop_rows<RAGGED>(a, slot, crop, ylo, g)) return;              // uniform
  const int x0 = g.x0, flip = g.flip, W = g.W;
  // byte offset of crop column j, channel 0, within a frame row: xb + xs*j
  const int xb = flip ? (W - 1 - x0) * 3 : x0 * 3, xs = flip ? -3 : 3;
  const uint8_t* fr = g.fr;

  // horizontal pass: item = (row, c, xg), xg fastest
  for (int it = tid; it < rows * 3 * nxg; it += 256) {
    const int xg = it % nxg, rc = it / nxg;
    const int c = rc % 3, row = rc / 3;
    const uint8_t* src = fr + (long)row * W * 3 + xb + c;
    const int4 xm = reinterpret_cast<const int4*>(a.xmin)[xg];
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < a.xtaps; ++i) {
      const int4 k = reinterpret_cast<const int4*>(a.xk + (long)i * Sp)[xg];
      a0 += k.x * (int)src[xs * clampi(xm.x + i, 0, a.cw - 1)];
      a1 += k.y * (int)src[xs * clampi(xm.y + i, 0, a.cw - 1)];
      a2 += k.z * (int)src[xs * clampi(xm.z + i, 0, a.cw - 1)];
      a3 += k.w * (int)src[xs * clampi(xm.w + i, 0, a.cw - 1)];
    }
    reinterpret_cast<unsigned*>(hrows)[(row * 3 + c) * nxg + xg] =
        fix8(a0) | (fix8(a1) << 8) | (fix8(a2) << 16) | (fix8(a3) << 24);
  }
  __syncthreads();

  // vertical pass: item = (r, c, xg), xg fastest
  const int clip = slot / a.T, t = slot % a.T;
  const bool vec = (a.S & 3) == 0 && (((uintptr_t)a.out) & 15) == 0;
  for (int it = tid; it < (r1 - r0) * 3 * nxg; it += 256) {
    const int xg = it % nxg, rc = it / nxg;
    const int c = rc % 3, r = r0 + rc / 3;
    const int ym = a.ymin[r] - ylo;
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < a.ytaps; ++i) {
      const int k = a.yk[(long)i * Sp + r];
      const unsigned w = reinterpret_cast<const unsigned*>(hrows)[(clampi(ym + i, 0, rows - 1) * 3 + c) * nxg + xg];
      a0 += k * (int)(w & 255u);
      a1 += k * (int)((w >> 8) & 255u);
      a2 += k * (int)((w >> 16) & 255u);
      a3 += k * (int)(w >> 24);
    }
    if (U8OUT) {
      const unsigned v[4] = {fix8(a0), fix8(a1), fix8(a2), fix8(a3)};
      uint8_t* dst = a.out8 + ((((long)crop * gridDim.y + slot) * a.S + r) * (long)a.S + xg * 4) * 3 + c;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xg * 4 + j < a.S) dst[3 * j] = (uint8_t)v[j];
      continue;
    }
    const float mean = a.mean[c], std = a.std[c];
    float4 o;
    o.x = norm1(__fdiv_rn((float)fix8(a0), 255.f), mean, std);
    o.y = norm1(__fdiv_rn((float)fix8(a1), 255.f), mean, std);
    o.z = norm1(__fdiv_rn((float)fix8(a2), 255.f), mean, std);
    o.w = norm1(__fdiv_rn((float)fix8(a3), 255.f), mean, std);
    float* dst = a.out + (((((long)crop * a.n_clips + clip) * 3 + c) * a.T + t) * a.S + r) * (long)a.S + xg * 4;
    if (vec) {
      *reinterpret_cast<float4*>(dst) = o;
    } else {
      const float v[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xg * 4 + j < a.S) dst[j] = v[j];
    }
  }
}

// ---- RandomSizedCrop boxes of a training batch (utils/augmentation.py:90-138) ---------------------------------------
// crop (x0, y0, w, h) -> Image.resize((S, S), BICUBIC): the body of stage_crops_kernel<true> with the box, its SIZE and
// its tables per output clip.  A descriptor per clip (device data, int32 x BOX_FIELDS) names the clip's first frame,
// its box and where its tables start in the two concatenated table buffers: per box and axis `min[Sp]` followed by
// `k[taps][Sp]`.  No flip here: the reference flips after the resize (kind 7 of the augment kernel below).
// The descriptors are device data like the tables: every field is clamped into the frame / the table buffers, so
// whatever they hold nothing is out of bounds (the entry point validates the host copy before the launch).
enum { BOX_FIRST = 0, BOX_FRAMES, BOX_X0, BOX_Y0, BOX_W, BOX_H, BOX_XOFF, BOX_YOFF, BOX_XTAPS, BOX_YTAPS, BOX_FIELDS };

// The RAGGED forms of the two box kernels (coclr_resize_boxes_ragged_u8, coclr_resize2_boxes_ragged): the frames lie in
// one flat byte buffer and differ in size from clip to clip.  A ragged descriptor is the plain one followed by
// RAG_FIELDS words: the byte offset of the clip's first frame (64 bits, low word first) and the W and H of its frames,
// which follow each other at W * H * 3 bytes rounded up to 16 (every frame starts aligned); `first` is not read.  The box is clamped to the clip's OWN frame, and a
// clip whose T frames do not lie inside the buffer of `nbytes` is skipped, so nothing is read outside it.
enum { RAG_OFF_LO = 0, RAG_OFF_HI, RAG_W, RAG_H, RAG_FIELDS };

struct RagFrame { const uint8_t* base; int W, H; };

template <bool RAGGED>
__device__ __forceinline__ bool clip_frame(const uint8_t* frames, long nbytes, int F, int H, int W, const int32_t* d,
                                           const int32_t* rag, int T, int t, RagFrame& o) {
  if (RAGGED) {
    o.W = clampi(rag[RAG_W], 1, kRagMaxSide);
    o.H = clampi(rag[RAG_H], 1, kRagMaxSide);
    const long fb = (long)o.W * o.H * 3, step = (fb + 15) & ~15L;
    const long off = (long)(((unsigned long)(unsigned)rag[RAG_OFF_HI] << 32) | (unsigned)rag[RAG_OFF_LO]);
    if (off < 0 || off > nbytes - (step * (T - 1) + fb)) return false;
    o.base = frames + off + step * t;
  } else {
    o.W = W;
    o.H = H;
    o.base = frames + (long)clampi(d[0] + t, 0, F - 1) * H * (long)W * 3;
  }
  return true;
}

struct BoxArgs {
  const uint8_t* frames; const int32_t* desc;
  const int32_t *xtab, *ytab;                // per box: min[Sp], k[taps][Sp]
  uint8_t* out8;                             // [n_clips*T][S][S][3]
  long nbytes;                               // ragged: bytes of `frames`
  int F, H, W, T, S, Sp, R, cap_rows, xlen, ylen;
};

template <bool RAGGED>
__global__ void __launch_bounds__(256)
resize_boxes_kernel(const BoxArgs a) {
  extern __shared__ __align__(16) uint8_t hrows[];      // [rows][3][Sp]
  const int tid = threadIdx.x;
  const int band = blockIdx.x, slot = blockIdx.y;
  const int clip = slot / a.T, t = slot % a.T;
  constexpr int fields = BOX_FIELDS + (RAGGED ? RAG_FIELDS : 0);
  const int32_t* d = a.desc + (long)clip * fields;
  const int Sp = a.Sp, nxg = Sp >> 2;
  RagFrame fm;
  if (!clip_frame<RAGGED>(a.frames, a.nbytes, a.F, a.H, a.W, d, d + BOX_FIELDS, a.T, t, fm)) return;   // uniform
  const int x0 = clampi(d[BOX_X0], 0, fm.W - 1), y0 = clampi(d[BOX_Y0], 0, fm.H - 1);
  const int cw = clampi(d[BOX_W], 1, fm.W - x0), ch = clampi(d[BOX_H], 1, fm.H - y0);
  const int xtaps = clampi(d[BOX_XTAPS], 1, min(64, a.xlen / Sp - 1));
  const int ytaps = clampi(d[BOX_YTAPS], 1, min(64, a.ylen / Sp - 1));
  const int32_t* xmin = a.xtab + clampi(d[BOX_XOFF] & ~3, 0, a.xlen - Sp * (1 + xtaps));
  const int32_t* ymin = a.ytab + clampi(d[BOX_YOFF] & ~3, 0, a.ylen - Sp * (1 + ytaps));
  const int32_t *xk = xmin + Sp, *yk = ymin + Sp;
  const int r0 = band * a.R, r1 = min(r0 + a.R, a.S);                  // output rows [r0, r1)
  const int ylo = clampi(ymin[r0], 0, ch - 1);
  const int rows = min(clampi(ymin[r1 - 1] + ytaps, ylo + 1, ch) - ylo, a.cap_rows);
  const uint8_t* fr = fm.base + (long)(y0 + ylo) * fm.W * 3 + x0 * 3;

  // horizontal pass: item = (row, c, xg), xg fastest
  for (int it = tid; it < rows * 3 * nxg; it += 256) {
    const int xg = it % nxg, rc = it / nxg;
    const int c = rc % 3, row = rc / 3;
    const uint8_t* src = fr + (long)row * fm.W * 3 + c;
    const int4 xm = reinterpret_cast<const int4*>(xmin)[xg];
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < xtaps; ++i) {
      const int4 k = reinterpret_cast<const int4*>(xk + (long)i * Sp)[xg];
      a0 += k.x * (int)src[3 * clampi(xm.x + i, 0, cw - 1)];
      a1 += k.y * (int)src[3 * clampi(xm.y + i, 0, cw - 1)];
      a2 += k.z * (int)src[3 * clampi(xm.z + i, 0, cw - 1)];
      a3 += k.w * (int)src[3 * clampi(xm.w + i, 0, cw - 1)];
    }
    reinterpret_cast<unsigned*>(hrows)[(row * 3 + c) * nxg + xg] =
        fix8(a0) | (fix8(a1) << 8) | (fix8(a2) << 16) | (fix8(a3) << 24);
  }
  __syncthreads();

  // vertical pass: item = (r, c, xg), xg fastest
  for (int it = tid; it < (r1 - r0) * 3 * nxg; it += 256) {
    const int xg = it % nxg, rc = it / nxg;
    const int c = rc % 3, r = r0 + rc / 3;
    const int ym = ymin[r] - ylo;
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < ytaps; ++i) {
      const int k = yk[(long)i * Sp + r];
      const unsigned w = reinterpret_cast<const unsigned*>(hrows)[(clampi(ym + i, 0, rows - 1) * 3 + c) * nxg + xg];
      a0 += k * (int)(w & 255u);
      a1 += k * (int)((w >> 8) & 255u);
      a2 += k * (int)((w >> 16) & 255u);
      a3 += k * (int)(w >> 24);
    }
    const unsigned v[4] = {fix8(a0), fix8(a1), fix8(a2), fix8(a3)};
    uint8_t* dst = a.out8 + ((((long)slot * a.S + r) * (long)a.S + xg * 4) * 3 + c);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (xg * 4 + j < a.S) dst[3 * j] = (uint8_t)v[j];
  }
}

// ---- the classifier's crop chain (eval/main_classifier.py:729-744; utils/augmentation.py:21-58,90-146) -------------
// RandomSizedCrop(size, consistent=True) -> Scale(img_dim): TWO of PIL's 8-bit resizes per frame, the first either of
// a drawn box to size x size or (the fallback, after ten draws that do not fit) of the whole frame to (ow, oh) of which
// CenterCrop keeps a size x size window.  Both are "resample region (x0, y0, w, h) and keep size columns / rows of the
// result": the window is in the TABLES (the host hands over the window's columns / rows of resample_tables(w, ow) /
// (h, oh)), so the kernel sees one form.  The second resize is size -> S on both axes, one table for every clip.
// Four passes, each rounded and clamped to bytes on its own as PIL does: H1, V1 (the size x size image), H2, V2.
// One workgroup per (band of R rows of the S x S output, slot = (clip, t)) with everything between the source frame
// and the output in LDS:
//   one   [rows1][3][P]   H1 of the source rows the band's intermediate rows need (P = size rounded up to 4)
//   mid   [arows][3][P]   V1: the band's rows of the size x size image
//   one   [arows][3][Sp]  H2 of those rows (`one` again: H1's rows are dead after V1)
// and V2 stores bytes (the input of coclr_augment_clips) or normalised fp32 with the arithmetic of stage_crops_kernel.
// The descriptors and all tables are device data: every index derived from them is clamped into the region, the
// staged rows or the table buffers (the entry point validates the host copy of the descriptors before the launch).
enum { CLS_FIRST = 0, CLS_FRAMES, CLS_X0, CLS_Y0, CLS_W, CLS_H, CLS_OW, CLS_OH, CLS_CX, CLS_CY, CLS_XOFF, CLS_YOFF,
       CLS_XTAPS, CLS_YTAPS, CLS_FIELDS };
constexpr int kClsThreads = 512;
constexpr int kClsMaxSide = 224;             // size and S: what coclr_augment_clips takes
constexpr int kClsLdsTwo = 80 * 1024;        // a band's footprint that leaves room for two workgroups per CU
constexpr int kClsLdsMax = 160 * 1024;

struct Resize2Args {
  const uint8_t* frames; const int32_t* desc;
  const int32_t *xtab, *ytab;                // stage 1, per clip: min[P], k[taps][P] of the window's columns / rows
  const int32_t* tab2;                       // stage 2, shared: min[Sp], k[taps2][Sp]
  uint8_t* out8;                             // [n_clips*T][S][S][3]
  float* out;                                // [n_clips][3][T][S][S], normalised
  float mean[3], std[3];
  long nbytes;                               // ragged: bytes of `frames`
  int F, H, W, T, size, P, S, Sp, taps2, R, cap1, capA, xlen, ylen;
};

template <bool U8OUT, bool RAGGED>
__global__ void __launch_bounds__(kClsThreads)
resize2_boxes_kernel(const Resize2Args a) {
  extern __shared__ __align__(16) uint8_t lds2[];
  const int tid = threadIdx.x;
  const int band = blockIdx.x, slot = blockIdx.y;
  const int clip = slot / a.T, t = slot % a.T;
  constexpr int fields = CLS_FIELDS + (RAGGED ? RAG_FIELDS : 0);
  const int32_t* d = a.desc + (long)clip * fields;
  const int P = a.P, nx1 = P >> 2, Sp = a.Sp, nx2 = Sp >> 2, size = a.size;
  RagFrame fm;
  if (!clip_frame<RAGGED>(a.frames, a.nbytes, a.F, a.H, a.W, d, d + CLS_FIELDS, a.T, t, fm)) return;   // uniform
  const int x0 = clampi(d[CLS_X0], 0, fm.W - 1), y0 = clampi(d[CLS_Y0], 0, fm.H - 1);
  const int cw = clampi(d[CLS_W], 1, fm.W - x0), ch = clampi(d[CLS_H], 1, fm.H - y0);
  const int xtaps = clampi(d[CLS_XTAPS], 1, min(64, a.xlen / P - 1));
  const int ytaps = clampi(d[CLS_YTAPS], 1, min(64, a.ylen / P - 1));
  const int32_t* xmin = a.xtab + clampi(d[CLS_XOFF] & ~3, 0, a.xlen - P * (1 + xtaps));
  const int32_t* ymin = a.ytab + clampi(d[CLS_YOFF] & ~3, 0, a.ylen - P * (1 + ytaps));
  const int32_t *xk = xmin + P, *yk = ymin + P;
  const int32_t *min2 = a.tab2, *k2 = a.tab2 + Sp;
  const int taps2 = a.taps2;
  const int r0 = band * a.R, r1 = min(r0 + a.R, a.S);                  // output rows [r0, r1)
  // the band's rows [alo, alo + arows) of the size x size image, and their source rows [ylo, ylo + rows1) of the region
  const int alo = clampi(min2[r0], 0, size - 1);
  const int arows = min(clampi(min2[r1 - 1] + taps2, alo + 1, size) - alo, a.capA);
  const int ylo = clampi(ymin[alo], 0, ch - 1);
  const int rows1 = min(clampi(ymin[alo + arows - 1] + ytaps, ylo + 1, ch) - ylo, a.cap1);
  unsigned* one = reinterpret_cast<unsigned*>(lds2);
  const int one_bytes = max(a.cap1 * 3 * P, a.capA * 3 * Sp);
  unsigned* mid = reinterpret_cast<unsigned*>(lds2 + one_bytes);
  const uint8_t* fr = fm.base + (long)(y0 + ylo) * fm.W * 3 + x0 * 3;

  // H1: item = (row, c, xg), xg fastest
  for (int it = tid; it < rows1 * 3 * nx1; it += kClsThreads) {
    const int xg = it % nx1, rc = it / nx1;
    const int c = rc % 3, row = rc / 3;
    const uint8_t* src = fr + (long)row * fm.W * 3 + c;
    const int4 xm = reinterpret_cast<const int4*>(xmin)[xg];
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < xtaps; ++i) {
      const int4 k = reinterpret_cast<const int4*>(xk + (long)i * P)[xg];
      a0 += k.x * (int)src[3 * clampi(xm.x + i, 0, cw - 1)];
      a1 += k.y * (int)src[3 * clampi(xm.y + i, 0, cw - 1)];
      a2 += k.z * (int)src[3 * clampi(xm.z + i, 0, cw - 1)];
      a3 += k.w * (int)src[3 * clampi(xm.w + i, 0, cw - 1)];
    }
    one[(row * 3 + c) * nx1 + xg] = fix8(a0) | (fix8(a1) << 8) | (fix8(a2) << 16) | (fix8(a3) << 24);
  }
  __syncthreads();

  // V1: item = (ar, c, xg)
  for (int it = tid; it < arows * 3 * nx1; it += kClsThreads) {
    const int xg = it % nx1, rc = it / nx1;
    const int c = rc % 3, ar = rc / 3;
    const int ym = ymin[alo + ar] - ylo;
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < ytaps; ++i) {
      const int k = yk[(long)i * P + alo + ar];
      const unsigned w = one[(clampi(ym + i, 0, rows1 - 1) * 3 + c) * nx1 + xg];
      a0 += k * (int)(w & 255u);
      a1 += k * (int)((w >> 8) & 255u);
      a2 += k * (int)((w >> 16) & 255u);
      a3 += k * (int)(w >> 24);
    }
    mid[(ar * 3 + c) * nx1 + xg] = fix8(a0) | (fix8(a1) << 8) | (fix8(a2) << 16) | (fix8(a3) << 24);
  }
  __syncthreads();                                         // and H1's rows are dead: `one` is free

  // H2: item = (ar, c, xg) over the S output columns
  const uint8_t* midb = reinterpret_cast<const uint8_t*>(mid);
  for (int it = tid; it < arows * 3 * nx2; it += kClsThreads) {
    const int xg = it % nx2, rc = it / nx2;
    const uint8_t* src = midb + rc * P;
    const int4 xm = reinterpret_cast<const int4*>(min2)[xg];
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < taps2; ++i) {
      const int4 k = reinterpret_cast<const int4*>(k2 + (long)i * Sp)[xg];
      a0 += k.x * (int)src[clampi(xm.x + i, 0, size - 1)];
      a1 += k.y * (int)src[clampi(xm.y + i, 0, size - 1)];
      a2 += k.z * (int)src[clampi(xm.z + i, 0, size - 1)];
      a3 += k.w * (int)src[clampi(xm.w + i, 0, size - 1)];
    }
    one[rc * nx2 + xg] = fix8(a0) | (fix8(a1) << 8) | (fix8(a2) << 16) | (fix8(a3) << 24);
  }
  __syncthreads();

  // V2: item = (r, c, xg)
  const bool vec = (a.S & 3) == 0 && (((uintptr_t)a.out) & 15) == 0;
  for (int it = tid; it < (r1 - r0) * 3 * nx2; it += kClsThreads) {
    const int xg = it % nx2, rc = it / nx2;
    const int c = rc % 3, r = r0 + rc / 3;
    const int ym = min2[r] - alo;
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < taps2; ++i) {
      const int k = k2[(long)i * Sp + r];
      const unsigned w = one[(clampi(ym + i, 0, arows - 1) * 3 + c) * nx2 + xg];
      a0 += k * (int)(w & 255u);
      a1 += k * (int)((w >> 8) & 255u);
      a2 += k * (int)((w >> 16) & 255u);
      a3 += k * (int)(w >> 24);
    }
    if (U8OUT) {
      const unsigned v[4] = {fix8(a0), fix8(a1), fix8(a2), fix8(a3)};
      uint8_t* dst = a.out8 + ((((long)slot * a.S + r) * (long)a.S + xg * 4) * 3 + c);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xg * 4 + j < a.S) dst[3 * j] = (uint8_t)v[j];
      continue;
    }
    const float mean = a.mean[c], std = a.std[c];
    float4 o;
    o.x = norm1(__fdiv_rn((float)fix8(a0), 255.f), mean, std);
    o.y = norm1(__fdiv_rn((float)fix8(a1), 255.f), mean, std);
    o.z = norm1(__fdiv_rn((float)fix8(a2), 255.f), mean, std);
    o.w = norm1(__fdiv_rn((float)fix8(a3), 255.f), mean, std);
    float* dst = a.out + ((((long)clip * 3 + c) * a.T + t) * a.S + r) * (long)a.S + xg * 4;
    if (vec) {
      *reinterpret_cast<float4*>(dst) = o;
    } else {
      const float v[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xg * 4 + j < a.S) dst[j] = v[j];
    }
  }
}

// ---- ColorJitter / RandomGray on uint8 frames (utils/augmentation.py:179-320, through torchvision 0.5's
// functional on PIL: ImageEnhance.Brightness/Contrast/Color, convert('HSV') + uint8 add + convert('RGB')) ----------
// One workgroup owns one frame and runs its group's program (up to 8 ops, device tables) on the frame's bytes in
// PIL's own arithmetic, every operation rounded on its own: integers for L, fp32 for Image.blend, fp32 and double
// for the HSV round trip exactly where PIL's C uses float and double.  A lane always works on the same items
// (four consecutive pixels = three dwords), so pointwise ops chain in registers with no barrier.  Only contrast
// needs the whole frame -- the mean of L over the frame AS IT IS at that point of the program -- so the program
// is cut at every contrast op: a pass applies the ops up to the next contrast, parks the bytes in LDS
// ([item][3] dwords: a lane's stride of 3 dwords is odd, no bank conflict) while summing L in integers (exact and
// order-independent: sum < 2^24 for H*W <= 224*224), and after one workgroup reduction the next pass starts with
// that contrast.  The last pass converts with the arithmetic of stage_crops_kernel and stores 16 bytes along x
// into (clip, 3, T, H, W).  A program without contrast is one pass, global to global, and asks for no LDS.
// The tables are device data: an unknown kind does nothing, a gray channel is clamped, a hue shift is taken mod
// 256, and contrast is ignored when the launch brought no LDS -- whatever they hold, nothing is out of bounds.
//
// The augment form (AUG, coclr_augment_clips) adds the two ops the training transform needs:
//   blur  ImageFilter.GaussianBlur on 8-bit pixels = three box blurs along x, then three along y, each rounded to
//         bytes: out = (ww * sum_{|d| <= r} x[i+d] + fw * (x[i-r-1] + x[i+r+1]) + 2^23) >> 24 in uint32, indices
//         clamped to the line (PIL's edge replication), r = int(r_f), ww = uint32(2^24 / (2 r_f + 1)) in fp32,
//         fw = (2^24 - (2r+1) ww) / 2; the parameter is r_f, the fp32 box radius the host derived from sigma.
//         It is a whole-frame op like contrast: the program is cut there too, the bytes are parked, and six line
//         passes run on the parked frame IN PLACE -- a lane computes all its items (up to 13 x 3 dwords at
//         224 x 224) into registers, barrier, writes them, barrier: the frame fills the LDS, there is no second
//         buffer.  A lane keeps its items (four pixels consecutive along x) in BOTH directions, so its LDS address
//         is 12 * lane + a wave-uniform offset per tap: 3 dwords between lanes, odd, conflict-free for the byte
//         reads of the horizontal pass and the dword reads of the vertical one (W % 4 == 0: the rows above and
//         below an item are whole items; otherwise bytes).
//   flip  transpose(FLIP_LEFT_RIGHT).  It commutes with every other op bit for bit (pointwise ops and whole-frame
//         sums do not see the column; the blur's clamping is symmetric and its sums are integers), so an odd
//         number of flips in the program mirrors the column of the final store and nothing else.
enum { JIT_NOP = 0, JIT_BRIGHTNESS = 1, JIT_CONTRAST = 2, JIT_SATURATION = 3, JIT_HUE = 4, JIT_GRAY = 5, JIT_BLUR = 6,
       JIT_FLIP = 7 };
constexpr int kJitThreads = 512;
constexpr int kJitMaxPixels = 224 * 224;
constexpr int kAugThreads = 1024;            // the augment form: 13 items a lane to hold across the blur's barrier
constexpr int kBlurMaxIter = (kJitMaxPixels / 4 + kAugThreads - 1) / kAugThreads;
constexpr float kBlurMaxRadius = 16.f;

struct JitterArgs {
  const uint8_t* frames; const int32_t* kinds; const float* params; float* out;
  float mean[3], std[3];
  int HW, T, P, G, group_size, items, vec, use_lds, H, W;
};

__device__ __forceinline__ int lum8(int r, int g, int b) {          // PIL's convert('L')
  return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;
}

// Image.blend(degenerate d, image i, alpha a): one fp32 multiply and one fp32 add; PIL truncates when
// 0 <= a <= 1 (`inside`) and clips otherwise.
__device__ __forceinline__ int blend8(int d, int i, float a, bool inside) {
  const float t = __fadd_rn((float)d, __fmul_rn(a, (float)(i - d)));
  if (inside) return (int)t;
  return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}

// convert('HSV'), h = (h + shift) & 255, convert('RGB')
__device__ __forceinline__ void hue8(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  const int v = maxc;
  int uh = 0, us = 0;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = __fdiv_rn(cr, (float)maxc);
    const float rc = __fdiv_rn((float)(maxc - r), cr);
    const float gc = __fdiv_rn((float)(maxc - g), cr);
    const float bc = __fdiv_rn((float)(maxc - b), cr);
    float h;
    if (r == maxc) h = __fsub_rn(bc, gc);
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;                 // in [5/6, 11/6]: x - floor(x) is fmod(x, 1.0), exactly
    h = (float)(x - floor(x));
    uh = clampi((int)((double)h * 255.0), 0, 255);
    us = clampi((int)((double)s * 255.0), 0, 255);
  }
  uh = (uh + shift) & 255;
  if (us == 0) { r = g = b = v; return; }
  const double h6 = (double)uh * 6.0 / 255.0;
  const double fl = floor(h6);
  const float f = (float)(h6 - fl);
  const float fs = (float)((double)us / 255.0);
  const double vd = (double)v;
  const int p = clampi((int)round(vd * (1.0 - (double)fs)), 0, 255);
  const int q = clampi((int)round(vd * (1.0 - (double)fs * (double)f)), 0, 255);
  const int t = clampi((int)round(vd * (1.0 - (double)fs * (1.0 - (double)f))), 0, 255);
  switch ((int)fl % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// One of PIL's six box-blur line passes over the parked frame (bytes as they lie in memory), in place.
__device__ __forceinline__ void blur_pass(unsigned* parked, int tid, int items, int HW, int H, int W, bool vertical,
                                          int r, unsigned ww, unsigned fw) {
  const uint8_t* px = reinterpret_cast<const uint8_t*>(parked);
  // the six passes share every lane's pixel coordinates; held across all of them they cost more registers than the
  // divisions they save, so each pass derives its own from a width the compiler cannot see through
  asm volatile("" : "+s"(W));
  const bool rows_are_items = vertical && (W & 3) == 0;
  unsigned keep[kBlurMaxIter][3];
#pragma unroll
  for (int k = 0; k < kBlurMaxIter; ++k) {
    const int it = tid + k * kAugThreads;
    keep[k][0] = keep[k][1] = keep[k][2] = 0u;
    if (it < items) {
      unsigned acc[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) acc[e] = 1u << 23;
      int y = (it * 4) / W, x = it * 4 - y * W;
      if (rows_are_items) {
        for (int d = -r - 1; d <= r + 1; ++d) {
          const unsigned wgt = (d == -r - 1 || d == r + 1) ? fw : ww;
          const unsigned* s = parked + (long)((clampi(y + d, 0, H - 1) * W + x) >> 2) * 3;
          const unsigned w[3] = {s[0], s[1], s[2]};
#pragma unroll
          for (int e = 0; e < 12; ++e) acc[e] += wgt * ((w[e >> 2] >> (8 * (e & 3))) & 255u);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          while (x >= W) { x -= W; ++y; }
          if (it * 4 + q < HW) {
            const int n = vertical ? H : W, i = vertical ? y : x;
            const int stride = vertical ? W * 3 : 3, base = vertical ? x * 3 : y * W * 3;
            for (int d = -r - 1; d <= r + 1; ++d) {
              const unsigned wgt = (d == -r - 1 || d == r + 1) ? fw : ww;
              const uint8_t* s = px + base + clampi(i + d, 0, n - 1) * stride;
              acc[3 * q] += wgt * s[0]; acc[3 * q + 1] += wgt * s[1]; acc[3 * q + 2] += wgt * s[2];
            }
          }
          ++x;
        }
      }
#pragma unroll
      for (int e = 0; e < 3; ++e)
        keep[k][e] = (acc[4 * e] >> 24) | ((acc[4 * e + 1] >> 24) << 8) | ((acc[4 * e + 2] >> 24) << 16) |
                     ((acc[4 * e + 3] >> 24) << 24);
    }
    __builtin_amdgcn_sched_barrier(0);     // one item at a time: only the packed results stay live
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kBlurMaxIter; ++k) {
    const int it = tid + k * kAugThreads;
    if (it < items) { parked[it * 3] = keep[k][0]; parked[it * 3 + 1] = keep[k][1]; parked[it * 3 + 2] = keep[k][2]; }
  }
  __syncthreads();
}

template <bool AUG>
__global__ void __launch_bounds__(AUG ? kAugThreads : kJitThreads)
color_jitter_kernel(const JitterArgs a) {
  extern __shared__ __align__(16) unsigned parked[];      // [items][3]: four RGB pixels, as they lie in memory
  constexpr int NT = AUG ? kAugThreads : kJitThreads;
  __shared__ unsigned red[NT / 64];
  const int tid = threadIdx.x, n = blockIdx.x;
  const int grp = min(n / a.group_size, a.G - 1);
  const int32_t* kinds = a.kinds + (long)grp * a.P;
  const float* params = a.params + (long)grp * a.P;
  const uint8_t* src = a.frames + (long)n * a.HW * 3;
  const bool src4 = (((uintptr_t)src) & 3) == 0;
  const long plane = (long)a.T * a.HW;                              // one channel of one clip
  float* dst = a.out + (long)(n / a.T) * 3 * plane + (long)(n % a.T) * a.HW;
  bool mirror = false;
  if (AUG)
    for (int j = 0; j < a.P; ++j) mirror ^= kinds[j] == JIT_FLIP;
  int op = 0, m = 0;
  bool lead = false;                       // ops[op] is a contrast whose mean `m` is known
  for (int pass = 0;; ++pass) {
    // this pass runs ops [op, end): a contrast op ends a pass and, with its mean `m` known, begins the next; a
    // blur ends a pass, runs on the parked bytes, and the next pass begins behind it
    int end = op + (lead ? 1 : 0);
    while (end < a.P && !(a.use_lds && (kinds[end] == JIT_CONTRAST || (AUG && kinds[end] == JIT_BLUR)))) ++end;
    const bool last = end >= a.P;
    unsigned sum = 0;
    for (int it = tid; it < a.items; it += NT) {
      const bool full = it * 4 + 3 < a.HW;
      unsigned w[3] = {0u, 0u, 0u};
      if (pass > 0) {
        w[0] = parked[it * 3]; w[1] = parked[it * 3 + 1]; w[2] = parked[it * 3 + 2];
      } else if (src4 && full) {
        const unsigned* s4 = reinterpret_cast<const unsigned*>(src) + (long)it * 3;
        w[0] = s4[0]; w[1] = s4[1]; w[2] = s4[2];
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
          if (it * 4 + k / 3 < a.HW) w[k >> 2] |= (unsigned)src[(long)it * 12 + k] << (8 * (k & 3));
      }
      int c[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) c[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
      for (int j = op; j < end; ++j) {
        const int kind = kinds[j];
        const float prm = params[j];
        const bool inside = prm >= 0.f && prm <= 1.f;
        if (kind == JIT_BRIGHTNESS) {
#pragma unroll
          for (int k = 0; k < 12; ++k) c[k] = blend8(0, c[k], prm, inside);
        } else if (kind == JIT_CONTRAST) {
          if (lead && j == op) {
#pragma unroll
            for (int k = 0; k < 12; ++k) c[k] = blend8(m, c[k], prm, inside);
          }
        } else if (kind == JIT_SATURATION) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int L = lum8(c[3 * q], c[3 * q + 1], c[3 * q + 2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) c[3 * q + k] = blend8(L, c[3 * q + k], prm, inside);
          }
        } else if (kind == JIT_HUE) {
          const int shift = (int)prm & 255;
#pragma unroll
          for (int q = 0; q < 4; ++q) hue8(c[3 * q], c[3 * q + 1], c[3 * q + 2], shift);
        } else if (kind == JIT_GRAY) {
          const int ch = clampi((int)prm, 0, 2);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int v = ch == 0 ? c[3 * q] : ch == 1 ? c[3 * q + 1] : c[3 * q + 2];
            c[3 * q] = c[3 * q + 1] = c[3 * q + 2] = v;
          }
        }
      }
      if (!last) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (it * 4 + q < a.HW) sum += (unsigned)lum8(c[3 * q], c[3 * q + 1], c[3 * q + 2]);
#pragma unroll
        for (int k = 0; k < 3; ++k)
          parked[it * 3 + k] = (unsigned)c[4 * k] | ((unsigned)c[4 * k + 1] << 8) | ((unsigned)c[4 * k + 2] << 16) |
                               ((unsigned)c[4 * k + 3] << 24);
      } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float mean = a.mean[ch], std = a.std[ch];
          float4 o;
          o.x = norm1(__fdiv_rn((float)c[ch], 255.f), mean, std);
          o.y = norm1(__fdiv_rn((float)c[3 + ch], 255.f), mean, std);
          o.z = norm1(__fdiv_rn((float)c[6 + ch], 255.f), mean, std);
          o.w = norm1(__fdiv_rn((float)c[9 + ch], 255.f), mean, std);
          float* d = dst + ch * plane + (long)it * 4;
          if (AUG && mirror) {
            const float v[4] = {o.x, o.y, o.z, o.w};
            if (a.vec) {                   // W % 4 == 0: the four pixels share a row and land on 16 aligned bytes
              const int y = (it * 4) / a.W, x = it * 4 - y * a.W;
              o.x = v[3]; o.y = v[2]; o.z = v[1]; o.w = v[0];
              *reinterpret_cast<float4*>(dst + ch * plane + (long)y * a.W + (a.W - 4 - x)) = o;
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (it * 4 + q < a.HW) {
                  const int y = (it * 4 + q) / a.W, x = it * 4 + q - y * a.W;
                  dst[ch * plane + (long)y * a.W + (a.W - 1 - x)] = v[q];
                }
            }
          } else if (a.vec) {
            *reinterpret_cast<float4*>(d) = o;
          } else {
            const float v[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (it * 4 + q < a.HW) d[q] = v[q];
          }
        }
      }
    }
    if (last) break;
    if (AUG && kinds[end] == JIT_BLUR) {
      const float rf = fminf(fmaxf(params[end], 0.f), kBlurMaxRadius);       // NaN -> 0
      const int r = (int)rf;
      const unsigned ww = (unsigned)__fdiv_rn(16777216.f, __fadd_rn(__fmul_rn(rf, 2.f), 1.f));
      const unsigned fw = ((1u << 24) - (unsigned)(2 * r + 1) * ww) >> 1;
      __syncthreads();                                     // every lane's bytes are parked
      for (int k = 0; k < 6; ++k) blur_pass(parked, tid, a.items, a.HW, a.H, a.W, k >= 3, r, ww, fw);
      op = end + 1;
      lead = false;
      continue;
    }
    // m = int(sum / count + 0.5) = (2*sum + count) / (2*count): sum <= 255 * 224 * 224 < 2^24
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    __syncthreads();                                       // the previous pass's readers of red[] are done
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) total += red[k];
    m = (int)((2u * total + (unsigned)a.HW) / (2u * (unsigned)a.HW));
    op = end;
    lead = true;
  }
}

}  // namespace

// Host-only plan queries (coclr_*_plan below): every launcher of this file computes one of these structs and launches
// from it, and the query reports the same struct without launching.

// Band height of the crop and box kernels: the most output rows whose source rows fit the LDS budget.  ymin is
// non-decreasing and advances by at most ch/S (+1 from truncation) per output row, so a band of R rows spans at most
// floor((R-1)*ch/S) + ytaps + 1 source rows; the kernel clamps to cap_rows whatever the tables say.
// False: one output row's taps do not fit 64 KiB of LDS.
struct BandPlan {
  int R, bands, cap_rows, clipped;           // clipped: cap_rows is the box height, not the bound
  long lds;                                  // dynamic LDS bytes: cap_rows * 3 * Sp
  int u8out, ragged, vec;                    // the instantiation; vec: 16-byte stores of the fp32 forms
};

static bool crop_band(int ch, int S, int Sp, int ytaps, BandPlan* p) {
  int R = 32, cap = 0, clipped = 0;
  for (;; R >>= 1) {
    cap = (int)(((long)(R - 1) * ch) / S) + ytaps + 2;
    clipped = cap > ch;
    if (clipped) cap = ch;
    const long bytes = (long)cap * 3 * Sp;
    if (bytes <= (R > 1 ? 32768 : 65536)) break;
    if (R == 1) return false;
  }
  p->R = R;
  p->bands = (S + R - 1) / R;
  p->cap_rows = cap;
  p->clipped = clipped;
  p->lds = (long)cap * 3 * Sp;
  return true;
}

static void report_band(const BandPlan& p, int32_t* out) {
  out[0] = p.R; out[1] = p.bands; out[2] = p.cap_rows; out[3] = (int32_t)p.lds; out[4] = p.clipped;
  out[5] = p.u8out; out[6] = p.ragged; out[7] = p.vec;
}

// What both crop entry points check and plan: `out` (fp32, with mean / std) or `out8` (the resized bytes).  Fills the
// kernel's arguments and the plan; no device pointer is read.
static int plan_crops(const uint8_t* frames, int F, int H, int W, const int32_t* slot_frame, int n_clips, int T,
                      const int32_t* crops, int n_crops, int cw, int ch, int S, const int32_t* xmin,
                      const int32_t* xk, int xtaps, const int32_t* ymin, const int32_t* yk, int ytaps,
                      const float* mean, const float* std, float* out, uint8_t* out8, CropArgs& a, BandPlan& p) {
  if (!frames || !slot_frame || !crops || !xmin || !xk || !ymin || !yk || (!out && !out8) || (out && (!mean || !std)))
    return COCLR_EINVAL;
  if (F < 1 || H < 1 || W < 1 || T < 1 || n_clips < 1 || S < 1 || S > 512 || cw < 1 || ch < 1)
    return COCLR_EINVAL;
  if (n_crops < 1 || n_crops > 16 || xtaps < 1 || xtaps > 64 || ytaps < 1 || ytaps > 64)
    return COCLR_EINVAL;
  if ((long)W * 3 * H > 0x7fffffffL || (long)n_clips * T > 65535) return COCLR_EINVAL;
  for (int k = 0; k < n_crops; ++k) {
    const int x0 = crops[3 * k], y0 = crops[3 * k + 1], flip = crops[3 * k + 2];
    if (x0 < 0 || y0 < 0 || (long)x0 + cw > W || (long)y0 + ch > H || (flip != 0 && flip != 1))
      return COCLR_EINVAL;
    a.crop[k][0] = x0; a.crop[k][1] = y0; a.crop[k][2] = flip;
  }
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = out ? mean[c] : 0.f; a.std[c] = out ? std[c] : 1.f;      // host arrays, read at call time
    if (a.std[c] == 0.f) return COCLR_EINVAL;
  }
  const int Sp = (S + 3) & ~3;
  if (!crop_band(ch, S, Sp, ytaps, &p)) return COCLR_EINVAL;
  if ((long)p.bands * n_clips * T * n_crops * 256 >= (1L << 32)) return COCLR_EINVAL;
  p.u8out = out ? 0 : 1; p.ragged = 0;
  p.vec = out && (S & 3) == 0 && (((uintptr_t)out) & 15) == 0;           // reported only: the kernel tests this itself
  a.frames = frames; a.slot_frame = slot_frame; a.xmin = xmin; a.xk = xk; a.ymin = ymin; a.yk = yk;
  a.out = out; a.out8 = out8;
  a.F = F; a.H = H; a.W = W; a.T = T; a.n_clips = n_clips; a.cw = cw; a.ch = ch; a.S = S; a.Sp = Sp;
  a.xtaps = xtaps; a.ytaps = ytaps; a.R = p.R; a.cap_rows = p.cap_rows;
  a.desc = nullptr; a.slot_off = nullptr; a.nbytes = 0;
  return 0;
}

static int launch_crops(const uint8_t* frames, int F, int H, int W, const int32_t* slot_frame, int n_clips, int T,
                        const int32_t* crops, int n_crops, int cw, int ch, int S, const int32_t* xmin,
                        const int32_t* xk, int xtaps, const int32_t* ymin, const int32_t* yk, int ytaps,
                        const float* mean, const float* std, float* out, uint8_t* out8, hipStream_t stream) {
  CropArgs a;
  BandPlan p;
  if (const int rc = plan_crops(frames, F, H, W, slot_frame, n_clips, T, crops, n_crops, cw, ch, S, xmin, xk, xtaps,
                                ymin, yk, ytaps, mean, std, out, out8, a, p))
    return rc;
  dim3 grid((unsigned)p.bands, (unsigned)(n_clips * T), (unsigned)n_crops);
  if (out) hipLaunchKernelGGL((stage_crops_kernel<false, false>), grid, dim3(256), (size_t)p.lds, stream, a);
  else hipLaunchKernelGGL((stage_crops_kernel<true, false>), grid, dim3(256), (size_t)p.lds, stream, a);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_stage_crops_plan(const uint8_t* frames, int F, int H, int W, const int32_t* slot_frame,
                                      int n_clips, int T, const int32_t* crops, int n_crops, int cw, int ch, int S,
                                      const int32_t* xmin, const int32_t* xk, int xtaps, const int32_t* ymin,
                                      const int32_t* yk, int ytaps, const float* mean, const float* std,
                                      uint8_t* out8, float* out, int32_t* plan) {
  if (!plan || (out8 == nullptr) == (out == nullptr)) return COCLR_EINVAL;
  CropArgs a;
  BandPlan p;
  if (const int rc = plan_crops(frames, F, H, W, slot_frame, n_clips, T, crops, n_crops, cw, ch, S, xmin, xk, xtaps,
                                ymin, yk, ytaps, mean, std, out, out8, a, p))
    return rc;
  report_band(p, plan);
  return 0;
}

extern "C" int coclr_stage_crops(const uint8_t* frames, int F, int H, int W, const int32_t* slot_frame,
                                 int n_clips, int T, const int32_t* crops, int n_crops, int cw, int ch, int S,
                                 const int32_t* xmin, const int32_t* xk, int xtaps, const int32_t* ymin,
                                 const int32_t* yk, int ytaps, const float* mean, const float* std, float* out,
                                 void* stream_) {
  if (!out || !mean || !std) return COCLR_EINVAL;
  return launch_crops(frames, F, H, W, slot_frame, n_clips, T, crops, n_crops, cw, ch, S, xmin, xk, xtaps, ymin,
                      yk, ytaps, mean, std, out, nullptr, (hipStream_t)stream_);
}

extern "C" int coclr_resize_crops_u8(const uint8_t* frames, int F, int H, int W, const int32_t* slot_frame,
                                     int n_clips, int T, const int32_t* crops, int n_crops, int cw, int ch, int S,
                                     const int32_t* xmin, const int32_t* xk, int xtaps, const int32_t* ymin,
                                     const int32_t* yk, int ytaps, uint8_t* out, void* stream_) {
  if (!out) return COCLR_EINVAL;
  return launch_crops(frames, F, H, W, slot_frame, n_clips, T, crops, n_crops, cw, ch, S, xmin, xk, xtaps, ymin,
                      yk, ytaps, nullptr, nullptr, nullptr, out, (hipStream_t)stream_);
}

// What coclr_stage_crops_ragged checks and plans; as plan_crops.
static int plan_crops_ragged(const uint8_t* frames, int64_t nbytes, const int32_t* desc, const int32_t* desc_host,
                             int n_clips, int T, const int64_t* slot_off, const int64_t* slot_off_host, int cw, int ch,
                             int S, const int32_t* xmin, const int32_t* xk, int xtaps, const int32_t* ymin,
                             const int32_t* yk, int ytaps, const float* mean, const float* std, uint8_t* out8,
                             float* out, CropArgs& a, BandPlan& p) {
  if (!frames || !desc || !desc_host || !slot_off || !slot_off_host || !xmin || !xk || !ymin || !yk)
    return COCLR_EINVAL;
  if ((out8 == nullptr) == (out == nullptr) || (out && (!mean || !std))) return COCLR_EINVAL;     // one of the two forms
  if ((((uintptr_t)frames) & 15) || (((uintptr_t)desc) & 3) || (((uintptr_t)slot_off) & 7) ||
      (((uintptr_t)xmin) & 15) || (((uintptr_t)xk) & 15) || (((uintptr_t)ymin) & 3) || (((uintptr_t)yk) & 3) ||
      (((uintptr_t)out) & 3))
    return COCLR_EINVAL;                                                  // 16-byte x-table loads
  if (nbytes < 1 || n_clips < 1 || T < 1 || S < 1 || S > 512 || cw < 1 || ch < 1) return COCLR_EINVAL;
  if (xtaps < 1 || xtaps > 64 || ytaps < 1 || ytaps > 64) return COCLR_EINVAL;
  if ((long)n_clips * T > 65535) return COCLR_EINVAL;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = out ? mean[c] : 0.f; a.std[c] = out ? std[c] : 1.f;      // host arrays, read at call time
    if (a.std[c] == 0.f) return COCLR_EINVAL;
  }
  for (int k = 0; k < n_clips; ++k) {
    const int32_t* d = desc_host + (long)k * CROP_FIELDS;
    const int W = d[CROP_W], H = d[CROP_H];
    if (W < 1 || H < 1 || W > kRagMaxSide || H > kRagMaxSide) return COCLR_EINVAL;
    if (d[CROP_X0] < 0 || d[CROP_Y0] < 0 || (long)d[CROP_X0] + cw > W || (long)d[CROP_Y0] + ch > H)
      return COCLR_EINVAL;                                                // the box is held to the clip's own frame
    if (d[CROP_FLIP] != 0 && d[CROP_FLIP] != 1) return COCLR_EINVAL;
    const long fb = (long)W * H * 3;
    for (int t = 0; t < T; ++t) {                                         // slots may repeat and share frames
      const long off = (long)slot_off_host[(long)k * T + t];
      if (off < 0 || (off & 15) || off > (long)nbytes - fb) return COCLR_EINVAL;
    }
  }
  const int Sp = (S + 3) & ~3;
  if (!crop_band(ch, S, Sp, ytaps, &p)) return COCLR_EINVAL;
  if ((long)p.bands * n_clips * T * 256 >= (1L << 32)) return COCLR_EINVAL;
  p.u8out = out ? 0 : 1; p.ragged = 1;
  p.vec = out && (S & 3) == 0 && (((uintptr_t)out) & 15) == 0;           // reported only: the kernel tests this itself
  a.frames = frames; a.slot_frame = nullptr; a.xmin = xmin; a.xk = xk; a.ymin = ymin; a.yk = yk;
  a.out = out; a.out8 = out8;
  a.F = 0; a.H = 0; a.W = 0; a.T = T; a.n_clips = n_clips; a.cw = cw; a.ch = ch; a.S = S; a.Sp = Sp;
  a.xtaps = xtaps; a.ytaps = ytaps; a.R = p.R; a.cap_rows = p.cap_rows;
  a.desc = desc; a.slot_off = slot_off; a.nbytes = (long)nbytes;
  for (int k = 0; k < 16; ++k) a.crop[k][0] = a.crop[k][1] = a.crop[k][2] = 0;
  return 0;
}

extern "C" int coclr_stage_crops_ragged(const uint8_t* frames, int64_t nbytes, const int32_t* desc,
                                        const int32_t* desc_host, int n_clips, int T, const int64_t* slot_off,
                                        const int64_t* slot_off_host, int cw, int ch, int S, const int32_t* xmin,
                                        const int32_t* xk, int xtaps, const int32_t* ymin, const int32_t* yk, int ytaps,
                                        const float* mean, const float* std, uint8_t* out8, float* out, void* stream_) {
  CropArgs a;
  BandPlan p;
  if (const int rc = plan_crops_ragged(frames, nbytes, desc, desc_host, n_clips, T, slot_off, slot_off_host, cw, ch, S,
                                       xmin, xk, xtaps, ymin, yk, ytaps, mean, std, out8, out, a, p))
    return rc;
  const dim3 grid((unsigned)p.bands, (unsigned)(n_clips * T));
  const hipStream_t stream = (hipStream_t)stream_;
  if (out) hipLaunchKernelGGL((stage_crops_kernel<false, true>), grid, dim3(256), (size_t)p.lds, stream, a);
  else hipLaunchKernelGGL((stage_crops_kernel<true, true>), grid, dim3(256), (size_t)p.lds, stream, a);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_stage_crops_ragged_plan(const uint8_t* frames, int64_t nbytes, const int32_t* desc,
                                             const int32_t* desc_host, int n_clips, int T, const int64_t* slot_off,
                                             const int64_t* slot_off_host, int cw, int ch, int S, const int32_t* xmin,
                                             const int32_t* xk, int xtaps, const int32_t* ymin, const int32_t* yk,
                                             int ytaps, const float* mean, const float* std, uint8_t* out8, float* out,
                                             int32_t* plan) {
  if (!plan) return COCLR_EINVAL;
  CropArgs a;
  BandPlan p;
  if (const int rc = plan_crops_ragged(frames, nbytes, desc, desc_host, n_clips, T, slot_off, slot_off_host, cw, ch, S,
                                       xmin, xk, xtaps, ymin, yk, ytaps, mean, std, out8, out, a, p))
    return rc;
  report_band(p, plan);
  return 0;
}

// What a program launch does.  cuts: contrast and blur ops of the longest program (a pass ends at each).
struct JitterPlan { int aug, use_lds, items, per_lane, vec, cuts; long lds; };

// What both program entry points check and plan; `aug` admits kinds 6 (blur) and 7 (flip) and runs the augment form.
static int plan_jitter(bool aug, const uint8_t* frames, int N, int H, int W, int T, const int32_t* kinds,
                       const float* params, const int32_t* kinds_host, const float* params_host, int G, int P,
                       int group_size, const float* mean, const float* std, float* out, JitterArgs& a, JitterPlan& p) {
  if (!frames || !kinds || !params || !kinds_host || !params_host || !mean || !std || !out) return COCLR_EINVAL;
  if (N < 1 || H < 1 || W < 1 || T < 1 || G < 1 || P < 1 || P > 8 || group_size < 1) return COCLR_EINVAL;
  if (N % T != 0 || (long)G * group_size < N) return COCLR_EINVAL;
  if ((long)H * W > kJitMaxPixels) return COCLR_EINVAL;     // the frame's bytes must fit one workgroup's LDS
  bool whole = false;                                       // an op that needs the whole frame: contrast, blur
  int cuts = 0, run = 0;
  for (long i = 0; i < (long)G * P; ++i) {
    const int kind = kinds_host[i];
    const float v = params_host[i];
    if (kind < JIT_NOP || kind > (aug ? JIT_FLIP : JIT_GRAY)) return COCLR_EINVAL;
    if (kind >= JIT_BRIGHTNESS && kind <= JIT_SATURATION && !(v - v == 0.f)) return COCLR_EINVAL;   // NaN, inf
    if (kind == JIT_HUE && !(v >= 0.f && v <= 255.f && v == (float)(int)v)) return COCLR_EINVAL;
    if (kind == JIT_GRAY && !(v == 0.f || v == 1.f || v == 2.f)) return COCLR_EINVAL;
    if (kind == JIT_BLUR && !(v >= 0.f && v <= kBlurMaxRadius)) return COCLR_EINVAL;                // NaN too
    whole = whole || kind == JIT_CONTRAST || kind == JIT_BLUR;
    if (i % P == 0) run = 0;
    run += kind == JIT_CONTRAST || kind == JIT_BLUR;
    cuts = run > cuts ? run : cuts;
  }
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean[c]; a.std[c] = std[c];             // host arrays, read at call time
    if (a.std[c] == 0.f) return COCLR_EINVAL;
  }
  a.frames = frames; a.kinds = kinds; a.params = params; a.out = out;
  a.HW = H * W; a.T = T; a.P = P; a.G = G; a.group_size = group_size; a.H = H; a.W = W;
  a.items = (a.HW + 3) / 4;
  a.vec = (W & 3) == 0 && (((uintptr_t)out) & 15) == 0;
  a.use_lds = whole ? 1 : 0;
  const int nt = aug ? kAugThreads : kJitThreads;
  p.aug = aug; p.use_lds = a.use_lds; p.items = a.items; p.per_lane = (a.items + nt - 1) / nt; p.vec = a.vec;
  p.cuts = cuts; p.lds = whole ? (long)a.items * 12 : 0;
  return 0;
}

static int launch_jitter(bool aug, const uint8_t* frames, int N, int H, int W, int T, const int32_t* kinds,
                         const float* params, const int32_t* kinds_host, const float* params_host, int G, int P,
                         int group_size, const float* mean, const float* std, float* out, hipStream_t stream) {
  JitterArgs a;
  JitterPlan p;
  if (const int rc = plan_jitter(aug, frames, N, H, W, T, kinds, params, kinds_host, params_host, G, P, group_size,
                                 mean, std, out, a, p))
    return rc;
  const size_t lds = (size_t)p.lds;
  if (p.use_lds) {                                       // 224 x 224 x 3 = 147 KiB of the CU's 160
    static std::atomic<uint64_t> attr_done{0}, attr_done_aug{0};
    if (aug)
      COCLR_RETURN_IF(ensure_dyn_lds(reinterpret_cast<const void*>(color_jitter_kernel<true>), kJitMaxPixels * 3,
                                     attr_done_aug));
    else
      COCLR_RETURN_IF(ensure_dyn_lds(reinterpret_cast<const void*>(color_jitter_kernel<false>), kJitMaxPixels * 3,
                                     attr_done));
  }
  if (aug) hipLaunchKernelGGL(color_jitter_kernel<true>, dim3((unsigned)N), dim3(kAugThreads), lds, stream, a);
  else hipLaunchKernelGGL(color_jitter_kernel<false>, dim3((unsigned)N), dim3(kJitThreads), lds, stream, a);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_jitter_plan(int aug, const uint8_t* frames, int N, int H, int W, int T, const int32_t* kinds,
                                 const float* params, const int32_t* kinds_host, const float* params_host, int G,
                                 int P, int group_size, const float* mean, const float* std, float* out,
                                 int32_t* plan) {
  if (!plan) return COCLR_EINVAL;
  JitterArgs a;
  JitterPlan p;
  if (const int rc = plan_jitter(aug != 0, frames, N, H, W, T, kinds, params, kinds_host, params_host, G, P,
                                 group_size, mean, std, out, a, p))
    return rc;
  plan[0] = p.aug; plan[1] = p.use_lds; plan[2] = (int32_t)p.lds; plan[3] = p.items; plan[4] = p.per_lane;
  plan[5] = p.vec; plan[6] = p.cuts;
  return 0;
}

extern "C" int coclr_color_jitter_clips(const uint8_t* frames, int N, int H, int W, int T, const int32_t* kinds,
                                        const float* params, const int32_t* kinds_host, const float* params_host,
                                        int G, int P, int group_size, const float* mean, const float* std,
                                        float* out, void* stream_) {
  return launch_jitter(false, frames, N, H, W, T, kinds, params, kinds_host, params_host, G, P, group_size, mean, std,
                       out, (hipStream_t)stream_);
}

extern "C" int coclr_augment_clips(const uint8_t* frames, int N, int H, int W, int T, const int32_t* kinds,
                                   const float* params, const int32_t* kinds_host, const float* params_host, int G,
                                   int P, int group_size, const float* mean, const float* std, float* out,
                                   void* stream_) {
  return launch_jitter(true, frames, N, H, W, T, kinds, params, kinds_host, params_host, G, P, group_size, mean, std,
                       out, (hipStream_t)stream_);
}

// What the ragged part of host descriptor `rag` must hold for a clip of T frames in a buffer of nbytes: an offset
// that is a multiple of 16 and T frames of a positive size inside the buffer.  Clips may share frames.
static bool rag_ok(const int32_t* rag, int T, int64_t nbytes, int* W, int* H) {
  const long off = (long)(((unsigned long)(unsigned)rag[RAG_OFF_HI] << 32) | (unsigned)rag[RAG_OFF_LO]);
  const int w = rag[RAG_W], h = rag[RAG_H];
  if (w < 1 || h < 1 || w > kRagMaxSide || h > kRagMaxSide || (long)w * 3 * h > 0x7fffffffL) return false;
  const long fb = (long)w * h * 3, step = (fb + 15) & ~15L;
  if (off < 0 || (off & 15) || off > nbytes - (step * (T - 1) + fb)) return false;
  *W = w;
  *H = h;
  return true;
}

// What both box entry points check and plan.  ragged: `desc` rows carry RAG_FIELDS more words, F / H / W are not used.
static int plan_boxes(bool ragged, const uint8_t* frames, int64_t nbytes, int F, int H, int W, const int32_t* desc,
                      const int32_t* desc_host, int n_clips, int T, int S, const int32_t* xtab, int64_t xlen,
                      const int32_t* ytab, int64_t ylen, uint8_t* out, BoxArgs& a, BandPlan& p) {
  if (!frames || !desc || !desc_host || !xtab || !ytab || !out) return COCLR_EINVAL;
  if (T < 1 || n_clips < 1 || S < 1 || S > 512) return COCLR_EINVAL;
  if (ragged) {
    if (nbytes < 1 || (((uintptr_t)frames) & 15) || (((uintptr_t)desc) & 3)) return COCLR_EINVAL;
  } else if (F < 1 || H < 1 || W < 1 || (long)W * 3 * H > 0x7fffffffL) {
    return COCLR_EINVAL;
  }
  if ((long)n_clips * T > 65535) return COCLR_EINVAL;
  const int fields = BOX_FIELDS + (ragged ? RAG_FIELDS : 0);
  if ((((uintptr_t)xtab) & 15) || (((uintptr_t)ytab) & 15)) return COCLR_EINVAL;       // 16-byte table loads
  const int Sp = (S + 3) & ~3;
  if (xlen < 2 * Sp || ylen < 2 * Sp || xlen > 0x7fffffffL || ylen > 0x7fffffffL) return COCLR_EINVAL;
  int hmax = 0, ytmax = 0;
  for (int k = 0; k < n_clips; ++k) {
    const int32_t* d = desc_host + (long)k * fields;
    if (d[BOX_FRAMES] != T) return COCLR_EINVAL;
    if (ragged) {
      if (!rag_ok(d + BOX_FIELDS, T, nbytes, &W, &H)) return COCLR_EINVAL;      // the box is held to the clip's own frame
    } else if (d[BOX_FIRST] < 0 || (long)d[BOX_FIRST] + T > F) {
      return COCLR_EINVAL;
    }
    if (d[BOX_X0] < 0 || d[BOX_Y0] < 0 || d[BOX_W] < 1 || d[BOX_H] < 1 || (long)d[BOX_X0] + d[BOX_W] > W ||
        (long)d[BOX_Y0] + d[BOX_H] > H)
      return COCLR_EINVAL;
    if (d[BOX_XTAPS] < 1 || d[BOX_XTAPS] > 64 || d[BOX_YTAPS] < 1 || d[BOX_YTAPS] > 64) return COCLR_EINVAL;
    if (d[BOX_XOFF] < 0 || (d[BOX_XOFF] & 3) || (long)d[BOX_XOFF] + (long)Sp * (1 + d[BOX_XTAPS]) > xlen)
      return COCLR_EINVAL;
    if (d[BOX_YOFF] < 0 || (d[BOX_YOFF] & 3) || (long)d[BOX_YOFF] + (long)Sp * (1 + d[BOX_YTAPS]) > ylen)
      return COCLR_EINVAL;
    hmax = d[BOX_H] > hmax ? d[BOX_H] : hmax;
    ytmax = d[BOX_YTAPS] > ytmax ? d[BOX_YTAPS] : ytmax;
  }
  // band height as in plan_crops, for the tallest box and the most taps of the launch: a band of any box then
  // spans no more source rows than that; the kernel clamps to cap_rows whatever the tables say
  if (!crop_band(hmax, S, Sp, ytmax, &p)) return COCLR_EINVAL;       // one output row's taps do not fit 64 KiB of LDS
  if ((long)p.bands * n_clips * T * 256 >= (1L << 32)) return COCLR_EINVAL;
  p.u8out = 1; p.ragged = ragged; p.vec = 0;
  a.frames = frames; a.desc = desc; a.xtab = xtab; a.ytab = ytab; a.out8 = out;
  a.F = F; a.H = H; a.W = W; a.T = T; a.S = S; a.Sp = Sp; a.R = p.R; a.cap_rows = p.cap_rows;
  a.xlen = (int)xlen; a.ylen = (int)ylen; a.nbytes = (long)nbytes;
  return 0;
}

static int launch_boxes(bool ragged, const uint8_t* frames, int64_t nbytes, int F, int H, int W, const int32_t* desc,
                        const int32_t* desc_host, int n_clips, int T, int S, const int32_t* xtab, int64_t xlen,
                        const int32_t* ytab, int64_t ylen, uint8_t* out, void* stream_) {
  BoxArgs a;
  BandPlan p;
  if (const int rc = plan_boxes(ragged, frames, nbytes, F, H, W, desc, desc_host, n_clips, T, S, xtab, xlen, ytab, ylen,
                                out, a, p))
    return rc;
  const dim3 grid((unsigned)p.bands, (unsigned)(n_clips * T));
  if (ragged)
    hipLaunchKernelGGL(resize_boxes_kernel<true>, grid, dim3(256), (size_t)p.lds, (hipStream_t)stream_, a);
  else
    hipLaunchKernelGGL(resize_boxes_kernel<false>, grid, dim3(256), (size_t)p.lds, (hipStream_t)stream_, a);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_resize_boxes_plan(int ragged, const uint8_t* frames, int64_t nbytes, int F, int H, int W,
                                       const int32_t* desc, const int32_t* desc_host, int n_clips, int T, int S,
                                       const int32_t* xtab, int64_t xlen, const int32_t* ytab, int64_t ylen,
                                       uint8_t* out, int32_t* plan) {
  if (!plan) return COCLR_EINVAL;
  BoxArgs a;
  BandPlan p;
  if (const int rc = plan_boxes(ragged != 0, frames, nbytes, F, H, W, desc, desc_host, n_clips, T, S, xtab, xlen, ytab,
                                ylen, out, a, p))
    return rc;
  report_band(p, plan);
  return 0;
}

extern "C" int coclr_resize_boxes_u8(const uint8_t* frames, int F, int H, int W, const int32_t* desc,
                                     const int32_t* desc_host, int n_clips, int T, int S, const int32_t* xtab,
                                     int64_t xlen, const int32_t* ytab, int64_t ylen, uint8_t* out, void* stream_) {
  return launch_boxes(false, frames, 0, F, H, W, desc, desc_host, n_clips, T, S, xtab, xlen, ytab, ylen, out, stream_);
}

extern "C" int coclr_resize_boxes_ragged_u8(const uint8_t* frames, int64_t nbytes, const int32_t* desc,
                                            const int32_t* desc_host, int n_clips, int T, int S, const int32_t* xtab,
                                            int64_t xlen, const int32_t* ytab, int64_t ylen, uint8_t* out,
                                            void* stream_) {
  return launch_boxes(true, frames, nbytes, 0, 0, 0, desc, desc_host, n_clips, T, S, xtab, xlen, ytab, ylen, out,
                      stream_);
}

// What a launch of the two-stage kernel does.  one_h1: H1's rows (cap1 * 3 * P), not H2's (capA * 3 * Sp), sized `one`;
// optin: the launch needs more than 64 KiB and raises the instantiation's dynamic-LDS limit.
struct Resize2Plan { int R, bands, cap1, capA, one_h1, optin, u8out, ragged, vec; long lds; };

// What both classifier entry points check and plan.  ragged: as plan_boxes.
static int plan_resize2(bool ragged, const uint8_t* frames, int64_t nbytes, int F, int H, int W, const int32_t* desc,
                        const int32_t* desc_host, int n_clips, int T, int size, int S, const int32_t* xtab,
                        int64_t xlen, const int32_t* ytab, int64_t ylen, const int32_t* tab2, int64_t len2,
                        int taps2, const float* mean, const float* std, uint8_t* out8, float* out, Resize2Args& a,
                        Resize2Plan& p) {
  if (!frames || !desc || !desc_host || !xtab || !ytab || !tab2) return COCLR_EINVAL;
  if ((out8 == nullptr) == (out == nullptr) || (out && (!mean || !std))) return COCLR_EINVAL;     // one of the two forms
  if (T < 1 || n_clips < 1 || S < 1 || size < 1) return COCLR_EINVAL;
  if (ragged) {
    if (nbytes < 1 || (((uintptr_t)frames) & 15) || (((uintptr_t)desc) & 3)) return COCLR_EINVAL;
  } else if (F < 1 || H < 1 || W < 1 || (long)W * 3 * H > 0x7fffffffL) {
    return COCLR_EINVAL;
  }
  if (S > kClsMaxSide || size > kClsMaxSide) return COCLR_EINVAL;
  if ((long)n_clips * T > 65535) return COCLR_EINVAL;
  const int fields = CLS_FIELDS + (ragged ? RAG_FIELDS : 0);
  if ((((uintptr_t)xtab) & 15) || (((uintptr_t)ytab) & 15) || (((uintptr_t)tab2) & 15)) return COCLR_EINVAL;
  const int P = (size + 3) & ~3, Sp = (S + 3) & ~3;
  if (xlen < 2 * P || ylen < 2 * P || xlen > 0x7fffffffL || ylen > 0x7fffffffL) return COCLR_EINVAL;
  if (taps2 < 1 || taps2 > 64 || len2 < (int64_t)Sp * (1 + taps2)) return COCLR_EINVAL;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = out ? mean[c] : 0.f; a.std[c] = out ? std[c] : 1.f;      // host arrays, read at call time
    if (a.std[c] == 0.f) return COCLR_EINVAL;
  }
  for (int k = 0; k < n_clips; ++k) {
    const int32_t* d = desc_host + (long)k * fields;
    if (d[CLS_FRAMES] != T) return COCLR_EINVAL;
    if (ragged) {
      if (!rag_ok(d + CLS_FIELDS, T, nbytes, &W, &H)) return COCLR_EINVAL;      // the region is held to the clip's own frame
    } else if (d[CLS_FIRST] < 0 || (long)d[CLS_FIRST] + T > F) {
      return COCLR_EINVAL;
    }
    if (d[CLS_X0] < 0 || d[CLS_Y0] < 0 || d[CLS_W] < 1 || d[CLS_H] < 1 || (long)d[CLS_X0] + d[CLS_W] > W ||
        (long)d[CLS_Y0] + d[CLS_H] > H)
      return COCLR_EINVAL;
    if (d[CLS_CX] < 0 || d[CLS_CY] < 0 || d[CLS_OW] < 1 || d[CLS_OH] < 1 || (long)d[CLS_CX] + size > d[CLS_OW] ||
        (long)d[CLS_CY] + size > d[CLS_OH])
      return COCLR_EINVAL;                                               // the window leaves the resampled region
    if (d[CLS_XTAPS] < 1 || d[CLS_XTAPS] > 64 || d[CLS_YTAPS] < 1 || d[CLS_YTAPS] > 64) return COCLR_EINVAL;
    if (d[CLS_XOFF] < 0 || (d[CLS_XOFF] & 3) || (long)d[CLS_XOFF] + (long)P * (1 + d[CLS_XTAPS]) > xlen)
      return COCLR_EINVAL;
    if (d[CLS_YOFF] < 0 || (d[CLS_YOFF] & 3) || (long)d[CLS_YOFF] + (long)P * (1 + d[CLS_YTAPS]) > ylen)
      return COCLR_EINVAL;
  }
  // Band height: the most output rows whose three LDS images fit.  Both row tables are non-decreasing and advance by
  // at most n_in / n_out (+1 from truncation) per row: a band of R output rows spans at most floor((R-1) size / S) +
  // taps2 + 2 rows of the size x size image, and capA of those at most floor((capA-1) h / oh) + ytaps + 2 source rows
  // of a clip; the kernel clamps to both caps whatever the tables say.  Up to 80 KiB two workgroups share a CU; a
  // single output row may take the whole 160 KiB.
  int R = 32, cap1 = 0, capA = 0, one_h1 = 0;
  long bytes = 0;
  for (;; R >>= 1) {
    capA = (int)(((long)(R - 1) * size) / S) + taps2 + 2;
    if (capA > size) capA = size;
    cap1 = 1;
    for (int k = 0; k < n_clips; ++k) {
      const int32_t* d = desc_host + (long)k * fields;
      long c1 = ((long)(capA - 1) * d[CLS_H]) / d[CLS_OH] + d[CLS_YTAPS] + 2;
      if (c1 > d[CLS_H]) c1 = d[CLS_H];
      if (c1 > cap1) cap1 = (int)c1;
    }
    one_h1 = (long)cap1 * 3 * P > (long)capA * 3 * Sp;
    const long one = one_h1 ? (long)cap1 * 3 * P : (long)capA * 3 * Sp;
    bytes = one + (long)capA * 3 * P;
    if (bytes <= (R > 1 ? kClsLdsTwo : kClsLdsMax)) break;
    if (R == 1) return COCLR_EINVAL;                   // one output row's halo does not fit the CU's LDS
  }
  const long bands = (S + R - 1) / R;
  if (bands * n_clips * T * kClsThreads >= (1L << 32)) return COCLR_EINVAL;
  p.R = R; p.bands = (int)bands; p.cap1 = cap1; p.capA = capA; p.one_h1 = one_h1; p.optin = bytes > 65536;
  p.u8out = out8 ? 1 : 0; p.ragged = ragged; p.lds = bytes;
  p.vec = out && (S & 3) == 0 && (((uintptr_t)out) & 15) == 0;           // reported only: the kernel tests this itself
  a.frames = frames; a.desc = desc; a.xtab = xtab; a.ytab = ytab; a.tab2 = tab2; a.out8 = out8; a.out = out;
  a.F = F; a.H = H; a.W = W; a.T = T; a.size = size; a.P = P; a.S = S; a.Sp = Sp; a.taps2 = taps2; a.R = R;
  a.cap1 = cap1; a.capA = capA; a.xlen = (int)xlen; a.ylen = (int)ylen; a.nbytes = (long)nbytes;
  return 0;
}

static int launch_resize2(bool ragged, const uint8_t* frames, int64_t nbytes, int F, int H, int W, const int32_t* desc,
                          const int32_t* desc_host, int n_clips, int T, int size, int S, const int32_t* xtab,
                          int64_t xlen, const int32_t* ytab, int64_t ylen, const int32_t* tab2, int64_t len2,
                          int taps2, const float* mean, const float* std, uint8_t* out8, float* out, void* stream_) {
  Resize2Args a;
  Resize2Plan p;
  if (const int rc = plan_resize2(ragged, frames, nbytes, F, H, W, desc, desc_host, n_clips, T, size, S, xtab, xlen,
                                  ytab, ylen, tab2, len2, taps2, mean, std, out8, out, a, p))
    return rc;
  static std::atomic<uint64_t> attr_u8{0}, attr_f32{0}, attr_rag_u8{0}, attr_rag_f32{0};
  const dim3 grid((unsigned)p.bands, (unsigned)(n_clips * T));
  const void* fn = ragged ? (out8 ? reinterpret_cast<const void*>(resize2_boxes_kernel<true, true>)
                                  : reinterpret_cast<const void*>(resize2_boxes_kernel<false, true>))
                          : (out8 ? reinterpret_cast<const void*>(resize2_boxes_kernel<true, false>)
                                  : reinterpret_cast<const void*>(resize2_boxes_kernel<false, false>));
  std::atomic<uint64_t>& done = ragged ? (out8 ? attr_rag_u8 : attr_rag_f32) : (out8 ? attr_u8 : attr_f32);
  if (p.optin) COCLR_RETURN_IF(ensure_dyn_lds(fn, kClsLdsMax, done));
  const hipStream_t st = (hipStream_t)stream_;
  const size_t bytes = (size_t)p.lds;
  if (ragged && out8) hipLaunchKernelGGL((resize2_boxes_kernel<true, true>), grid, dim3(kClsThreads), bytes, st, a);
  else if (ragged) hipLaunchKernelGGL((resize2_boxes_kernel<false, true>), grid, dim3(kClsThreads), bytes, st, a);
  else if (out8) hipLaunchKernelGGL((resize2_boxes_kernel<true, false>), grid, dim3(kClsThreads), bytes, st, a);
  else hipLaunchKernelGGL((resize2_boxes_kernel<false, false>), grid, dim3(kClsThreads), bytes, st, a);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_resize2_boxes_plan(int ragged, const uint8_t* frames, int64_t nbytes, int F, int H, int W,
                                        const int32_t* desc, const int32_t* desc_host, int n_clips, int T, int size,
                                        int S, const int32_t* xtab, int64_t xlen, const int32_t* ytab, int64_t ylen,
                                        const int32_t* tab2, int64_t len2, int taps2, const float* mean,
                                        const float* std, uint8_t* out8, float* out, int32_t* plan) {
  if (!plan) return COCLR_EINVAL;
  Resize2Args a;
  Resize2Plan p;
  if (const int rc = plan_resize2(ragged != 0, frames, nbytes, F, H, W, desc, desc_host, n_clips, T, size, S, xtab,
                                  xlen, ytab, ylen, tab2, len2, taps2, mean, std, out8, out, a, p))
    return rc;
  plan[0] = p.R; plan[1] = p.bands; plan[2] = p.cap1; plan[3] = p.capA; plan[4] = (int32_t)p.lds; plan[5] = p.one_h1;
  plan[6] = p.optin; plan[7] = p.u8out; plan[8] = p.ragged; plan[9] = p.vec;
  return 0;
}

extern "C" int coclr_resize2_boxes(const uint8_t* frames, int F, int H, int W, const int32_t* desc,
                                   const int32_t* desc_host, int n_clips, int T, int size, int S, const int32_t* xtab,
                                   int64_t xlen, const int32_t* ytab, int64_t ylen, const int32_t* tab2, int64_t len2,
                                   int taps2, const float* mean, const float* std, uint8_t* out8, float* out,
                                   void* stream_) {
  return launch_resize2(false, frames, 0, F, H, W, desc, desc_host, n_clips, T, size, S, xtab, xlen, ytab, ylen, tab2,
                        len2, taps2, mean, std, out8, out, stream_);
}

extern "C" int coclr_resize2_boxes_ragged(const uint8_t* frames, int64_t nbytes, const int32_t* desc,
                                          const int32_t* desc_host, int n_clips, int T, int size, int S,
                                          const int32_t* xtab, int64_t xlen, const int32_t* ytab, int64_t ylen,
                                          const int32_t* tab2, int64_t len2, int taps2, const float* mean,
                                          const float* std, uint8_t* out8, float* out, void* stream_) {
  return launch_resize2(true, frames, nbytes, 0, 0, 0, desc, desc_host, n_clips, T, size, S, xtab, xlen, ytab, ylen,
                        tab2, len2, taps2, mean, std, out8, out, stream_);
}

// What coclr_stage_clips checks and plans.  vec: THW is a multiple of the 16-byte access (so every run of either side
// starts where its buffer does, mod 16) and BOTH buffers start 16-byte aligned: the kernel loads and stores 16 bytes.
struct StagePlan { int u8, vec, gx; };

static int plan_stage(const void* frames, int from_u8, float* out, int B, int C, int S, int64_t THW, const float* mean,
                      const float* std, StageArgs& a, StagePlan& p) {
  if (B <= 0 || C <= 0 || C > 4 || S <= 0 || THW <= 0 || !frames || !out || !mean || !std)
    return COCLR_EINVAL;
  if ((long)B * C * S > 65535) return COCLR_EINVAL;
  a.in = frames; a.out = out; a.C = C; a.S = S; a.THW = (long)THW; a.from_u8 = from_u8;
  for (int c = 0; c < 4; ++c) {
    a.mean[c] = c < C ? mean[c] : 0.f;     // host arrays: three floats, read at call time
    a.std[c] = c < C ? std[c] : 1.f;
    if (c < C && a.std[c] == 0.f) return COCLR_EINVAL;
  }
  const long per_thread = from_u8 ? 16 : 4;
  long gx = (THW / per_thread + 255) / 256;
  if (gx < 1) gx = 1;
  if (gx > 64) gx = 64;
  a.vec = THW % per_thread == 0 && (((uintptr_t)frames) & 15) == 0 && (((uintptr_t)out) & 15) == 0;
  p.u8 = from_u8 != 0; p.vec = a.vec; p.gx = (int)gx;
  return 0;
}

extern "C" int coclr_stage_clips(const void* frames, int from_u8, float* out, int B, int C, int S,
                                 int64_t THW, const float* mean, const float* std, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  StageArgs a;
  StagePlan p;
  if (const int rc = plan_stage(frames, from_u8, out, B, C, S, THW, mean, std, a, p)) return rc;
  dim3 grid((unsigned)p.gx, (unsigned)(B * C * S));
  if (from_u8) hipLaunchKernelGGL(stage_clips_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(stage_clips_kernel<false>, grid, dim3(256), 0, stream, a);
  COCLR_LAUNCH_CHECK();
  return 0;
}

extern "C" int coclr_stage_clips_plan(const void* frames, int from_u8, float* out, int B, int C, int S, int64_t THW,
                                      const float* mean, const float* std, int32_t* plan) {
  if (!plan) return COCLR_EINVAL;
  StageArgs a;
  StagePlan p;
  if (const int rc = plan_stage(frames, from_u8, out, B, C, S, THW, mean, std, a, p)) return rc;
  plan[0] = p.u8; plan[1] = p.vec; plan[2] = p.gx;
  return 0;
}
