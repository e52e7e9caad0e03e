// Baseline JPEG frames -> uint8 (F, H, W, 3) on the device, bit-identical to libjpeg-turbo's default decoder
// (what PIL's Image.open(...).convert('RGB') returns; dataset/lmdb_dataset.py:37-38 of the reference).
// Three stages, one kernel each; the arithmetic lives in jpeg_core.h, shared with a host build:
//   1 entropy   one lane per (frame, restart segment): Huffman -> dequantised int16 coefficients
//   2 idct      one lane per 8x8 block: coefficients -> sample planes at the component's own resolution
//   4 colour    one lane per 16 output pixels of a row: chroma upsampling, YCbCr -> RGB, crop to (H, W)
// Huffman decoding is serial inside a restart segment.  A frame without restart markers is one lane of
// jpeg_entropy_kernel, or, with coclr_jpeg_decode_split's chunk_bytes > 0, one workgroup of
// jpeg_entropy_split_kernel: one lane per chunk of its bytes, decoded from guessed states until every chunk's
// entry is its predecessor's exit (jpeg_core.h), which is the serial decoder's result for any bytes.
// A store (coclr_jpeg_store_index, coclr_jpeg_decode_store, at the end) finds those states once per frame and keeps
// them: jpeg_store_index_kernel is the split kernel without its write pass, jpeg_entropy_store_kernel the write pass
// alone, a lane per chunk of any frame of the call.  The two kernels that find the states share one window loop
// (split_windows) and differ in what a lane does with its true entry.
// On the host every entry point is its own validation of its arguments and its choice of a geometry source; what they
// check alike (tables_ok, offsets_ok, frame_storage_ok), how frames are dealt to the two entropy kernels (plan_split,
// split_lanes, launch_entropy) and the stages themselves (run_stages) exist once.
#include "../../include/coclr_hip.h"
#include "common.h"
#include "jpeg_core.h"

namespace {

constexpr int JPEG_MAX_SIDE = 8192;

// Where a kernel gets a frame's geometry and storage from.  one_geom: the call's single geometry, by value, frame f
// at f times the per-frame sizes (coclr_jpeg_decode, coclr_jpeg_decode_split); the kernels read it where it lies, in
// the kernel arguments (a copy would cost LDS or scratch: it is indexed by component), and `store` is empty.
// table_geom<false>: per frame from the device table of coclr_jpeg_decode_ragged or coclr_jpeg_decode_store, built into
// the caller's `store`; a lane finds its frame by binary search over the prefix of lane counts.  False: skip.
// frame():  frame f -> its first block and first output byte (and, given a box to fill, its box)
// block():  lane id of the inverse DCT -> its frame's first block, and the block within the frame
// group():  lane id of the colour stage -> first block, the frame's first output byte, row and row group
// geom():   the geometry these found
// box, x0(), y0(), width():  what group() found besides: the colour stage's pixel origin in the frame and its output
//           row's width and pitch: 0, 0 and g.W, except for table_geom<true>, whose rows and groups are those of a BOX
//           of the frame.  The box is an object of its own so that it lives in registers: `store` is indexed by
//           component
// table_geom<true>: the same plus a box per frame (coclr_jpeg_decode_store_window; jpeg_core.h: JW_*).  block() maps a
// lane to a block of the box's MCU rectangle and returns its FULL-frame index, group() to a row and group of the box:
// the workspaces keep the full-frame layout, so the kernels address and compute as for a whole frame, on fewer lanes.
struct one_geom {
  static constexpr bool ragged = false;
  struct store {};
  struct box {};
  jc_geom g;
  __device__ const jc_geom& geom(const store&) const { return g; }
  __device__ bool frame(long f, store&, long* cb, long* ob) const {
    *cb = f * (long)g.nblocks;
    *ob = f * (long)g.H * g.W * 3;
    return true;
  }
  __device__ bool block(long id, store&, long* cb, int* blk) const {
    const long f = id / g.nblocks;
    *blk = (int)(id % g.nblocks);
    *cb = f * (long)g.nblocks;
    return true;
  }
  __device__ bool group(long id, int groups, store&, box&, long* cb, long* ob, int* y, int* xg) const {
    *xg = (int)(id % groups);
    const long row = id / groups;
    *y = (int)(row % g.H);
    const long f = row / g.H;
    *cb = f * (long)g.nblocks;
    *ob = f * (long)g.H * g.W * 3;
    return true;
  }
  __device__ bool vec_ok(int, long) const { return true; }
  __device__ int x0(const box&) const { return 0; }
  __device__ int y0(const box&) const { return 0; }
  __device__ int width(const store&, const box&) const { return g.W; }
};

template <bool WINDOWED>
struct table_geom {
  static constexpr bool ragged = true, windowed = WINDOWED;
  typedef jc_geom store;
  struct whole { static constexpr int x0 = 0, y0 = 0; };
  typedef std::conditional_t<WINDOWED, jc_window, whole> box;
  const int64_t* tab;        // [F][JR_FIELDS]; windowed: JR_OBYTE is the first of the box's 3 * w * h output bytes
  const int64_t* win;        // [F][JW_FIELDS]; unused unless windowed
  const int64_t* blocks;     // [F + 1] prefix of the frames' blocks, or of the blocks of the boxes' MCU rectangles
  const int64_t* rows;       // [F + 1] prefix of the frames' row groups, or the boxes'
  long F, coef_blocks, out_bytes;
  __device__ const jc_geom& geom(const store& o) const { return o; }
  __device__ bool frame(long f, store& o, box& w, long* cb, long* ob) const {
    if constexpr (WINDOWED) return jc_window_frame(tab, win, f, coef_blocks, out_bytes, JPEG_MAX_SIDE, o, w, cb, ob);
    else return jc_ragged_frame(tab, f, coef_blocks, out_bytes, JPEG_MAX_SIDE, o, cb, ob);
  }
  __device__ bool frame(long f, store& o, long* cb, long* ob) const {
    box w;
    return frame(f, o, w, cb, ob);
  }
  __device__ bool block(long id, store& o, long* cb, int* blk) const {
    const long f = jc_find_frame(blocks, F, id);
    box w;
    long ob;
    if (!frame(f, o, w, cb, &ob)) return false;
    const long local = id - blocks[f];
    if constexpr (WINDOWED) {
      if (local < 0 || local >= jc_window_blocks(o, w)) return false;
      *blk = jc_window_block(o, w, local);
    } else {
      if (local < 0 || local >= o.nblocks) return false;
      *blk = (int)local;
    }
    return true;
  }
  __device__ bool group(long id, int, store& o, box& w, long* cb, long* ob, int* y, int* xg) const {
    const long f = jc_find_frame(rows, F, id);
    if (!frame(f, o, w, cb, ob)) return false;
    const long local = id - rows[f];
    long n;
    if constexpr (WINDOWED) n = jc_window_row_groups(w);
    else n = jc_row_groups(o);
    if (local < 0 || local >= n) return false;
    const int groups = (width(o, w) + 15) / 16;
    *xg = (int)(local % groups);
    *y = (int)(local / groups);
    return true;
  }
  __device__ bool vec_ok(int width, long ob) const { return width % 16 == 0 && (ob & 15) == 0; }
  __device__ int x0(const box& w) const { return w.x0; }
  __device__ int y0(const box& w) const { return w.y0; }
  __device__ int width(const store& o, const box& w) const {
    if constexpr (WINDOWED) return w.w;
    else return o.W;
  }
};
typedef table_geom<false> ragged_geom;
typedef table_geom<true> window_geom;

// one wave per workgroup: with one lane per frame, 64 frames are all a CU gets, so the waves spread over the CUs
template <class GS>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ data, int data_len,
                                                          const int32_t* __restrict__ meta, int width, int F,
                                                          int maxseg, int multi_only, GS gs,
                                                          int16_t* __restrict__ coef, int32_t* __restrict__ status) {
  const long id = (long)blockIdx.x * 64 + threadIdx.x;
  const long f = id / maxseg;
  const int seg = (int)(id % maxseg);
  if (f >= F) return;
  typename GS::store gst;
  long cb, ob;
  if (!gs.frame(f, gst, &cb, &ob)) return;
  const jc_geom& g = gs.geom(gst);
  const int32_t* m = meta + f * width;
  if (multi_only && jc_segment_count(m, width, maxseg) == 1) return;      // jpeg_entropy_split_kernel's frames
  int s0, s1, m0, m1;
  if (!jc_segment_range(m, width, maxseg, data_len, seg, g, &s0, &s1, &m0, &m1)) return;
  const int st = jc_decode_segment(data, s0, s1, m, g, m0, m1, coef + cb * 64);
  if (st) atomicOr(&status[f], st);
}

// One window of blockDim.x chunks, from chunk w0, of a segment [s0, s1) whose tables are in LDS (`tab`), on the lanes
// of its workgroup; `first` is the true state at the window's start.  Relaxation, then the scan (see split_windows,
// which calls this window after window).  Afterwards `in` is the lane's TRUE entry and `out` its exit, `v` the
// inclusive and `e` the exclusive prefix over the window's lanes of {blocks completed (saturating at total), three DC
// sums}.  ex: [L][2], ps: [L][4] words of LDS.  Every barrier is on a workgroup-uniform path: all lanes call this
// together.
struct split_lane {
  bool live;
  int cend;
  jc_state in, out;
  uint32_t v[4], e[4];
};

__device__ __forceinline__ void split_window(const uint8_t* __restrict__ data, int s0, int s1, int chunk_bytes,
                                             const int32_t* tab, const jc_geom& g, long w0, long nchunks,
                                             const jc_state& first, uint32_t total, int32_t* ex, uint32_t* ps,
                                             split_lane& w) {
  const int t = threadIdx.x, L = blockDim.x;
  const bool live = w0 + t < nchunks;
  const int cend = live ? jc_chunk_end(s0, s1, chunk_bytes, w0 + t) : s1;
  jc_state in = t == 0 ? first : live ? jc_chunk_cold(data, s0, s1, chunk_bytes, w0 + t) : jc_state_past();
  jc_state out = in;
  int blocks = 0;
  uint32_t dcs[3] = {0, 0, 0};
  if (live) jc_chunk_scan(data, s1, cend, chunk_bytes, tab, g, in, &out, &blocks, dcs);
  ex[2 * t] = out.pos;
  ex[2 * t + 1] = jc_state_word(out);
  __syncthreads();
  for (int r = 0; r < L; ++r) {
    int changed = 0;
    jc_state left = in;
    if (live && t > 0) {
      left = jc_state_unpack(ex[2 * t - 2], ex[2 * t - 1], g);
      changed = left.pos != in.pos || jc_state_word(left) != jc_state_word(in);
    }
    __syncthreads();                                                       // all have read the previous round's exits
    if (changed) {
      in = left;
      jc_chunk_scan(data, s1, cend, chunk_bytes, tab, g, in, &out, &blocks, dcs);
      ex[2 * t] = out.pos;
      ex[2 * t + 1] = jc_state_word(out);
    }
    if (!__syncthreads_or(changed)) break;
  }
  uint32_t v[4] = {(uint32_t)blocks > total ? total : (uint32_t)blocks, dcs[0], dcs[1], dcs[2]};
  for (int i = 0; i < 4; ++i) ps[4 * t + i] = v[i];
  __syncthreads();
  for (int d = 1; d < L; d <<= 1) {                                        // inclusive prefix
    uint32_t a[4] = {0, 0, 0, 0};
    if (t >= d)
      for (int i = 0; i < 4; ++i) a[i] = ps[4 * (t - d) + i];
    __syncthreads();
    if (t >= d) {
      v[0] = jc_blocks_add(a[0], v[0], total);
      for (int i = 1; i < 4; ++i) v[i] += a[i];
      for (int i = 0; i < 4; ++i) ps[4 * t + i] = v[i];
    }
    __syncthreads();
  }
  w.live = live;
  w.cend = cend;
  w.in = in;
  w.out = out;
  for (int i = 0; i < 4; ++i) {
    w.v[i] = v[i];
    w.e[i] = t > 0 ? ps[4 * (t - 1) + i] : 0;                              // exclusive: the left neighbour's
  }
}

// A segment [s0, s1) of `total` blocks on the lanes of one workgroup, one lane per chunk of chunk_bytes raw bytes; a
// segment with more chunks than lanes is done in windows of blockDim.x chunks, in order, each starting from the
// converged exit of the one before.  Per window:
//   relaxation  every lane scans its chunk from a guessed state (lane 0 from the true one); then rounds: read the
//               left neighbour's exit, and scan again if it is not the entry this lane used.  A round in which no
//               lane changed has reached the serial decoder's states; blockDim.x rounds always suffice.
//   scan        exclusive prefix of blocks completed and DC sums over the lanes (Hillis-Steele in LDS)
//   emit        every lane with a chunk: emit(chunk, its end, its TRUE entry, blocks of the segment done before it,
//               the three DC sums there) -- jpeg_entropy_split_kernel decodes the chunk once more from that state,
//               jpeg_store_index_kernel stores the state
// Returns the first chunk no window reached: fewer than the segment has once only zero bits are left.
// LDS: `tab`, the segment's tables (JM_SEG words; the caller loads what it uses), per lane an exit state (ex, 2 words)
// and a scan element (ps, 4), and the carry from window to window (8: state (2), blocks, DC predictors (3)), which the
// caller sets to {s0, 0, ...} in front of the barrier that precedes the call: split_lds_bytes().  All lanes of the
// workgroup call this together, so every barrier is on a workgroup-uniform path.
template <class Emit>
__device__ __forceinline__ long split_windows(const uint8_t* __restrict__ data, int s0, int s1, int chunk_bytes,
                                              const int32_t* tab, const jc_geom& g, uint32_t total, int32_t* ex,
                                              uint32_t* ps, int32_t* carry, Emit emit) {
  const int t = threadIdx.x, L = blockDim.x;
  const long nchunks = jc_chunk_count(s0, s1, chunk_bytes);
  long w0 = 0;
  for (; w0 < nchunks; w0 += L) {
    const jc_state first = jc_state_unpack(carry[0], carry[1], g);
    if (first.pos == JC_PAST) break;                                       // uniform: nothing but zero bits is left
    const uint32_t block0 = (uint32_t)carry[2];
    const uint32_t dc0[3] = {(uint32_t)carry[3], (uint32_t)carry[4], (uint32_t)carry[5]};
    split_lane w;
    split_window(data, s0, s1, chunk_bytes, tab, g, w0, nchunks, first, total, ex, ps, w);
    if (w.live) {
      const uint32_t dc[3] = {dc0[0] + w.e[1], dc0[1] + w.e[2], dc0[2] + w.e[3]};
      emit(w0 + t, w.cend, w.in, jc_blocks_add(block0, w.e[0], total), dc);
    }
    __syncthreads();                                                       // the carry and the scan have been read
    if (t == L - 1) {
      carry[0] = w.out.pos;
      carry[1] = jc_state_word(w.out);
      carry[2] = (int32_t)jc_blocks_add(block0, w.v[0], total);
      for (int i = 0; i < 3; ++i) carry[3 + i] = (int32_t)(dc0[i] + w.v[1 + i]);
    }
    __syncthreads();
  }
  return w0;
}

// One workgroup per frame of ONE segment (the others return at once): split_windows, every chunk written from its
// true state to jc_decode_segment's addresses.  Dynamic LDS: split_lds_bytes().  Every barrier is on a
// workgroup-uniform path.
template <class GS>
__global__ __launch_bounds__(1024) void jpeg_entropy_split_kernel(const uint8_t* __restrict__ data, int data_len,
                                                                  const int32_t* __restrict__ meta, int width,
                                                                  int maxseg, int chunk_bytes, GS gs,
                                                                  int16_t* __restrict__ coef,
                                                                  int32_t* __restrict__ status) {
  extern __shared__ int32_t split_lds[];
  const int t = threadIdx.x, L = blockDim.x;
  const long f = blockIdx.x;
  // the whole workgroup is frame f: the ragged form builds its geometry once, in LDS, where the lanes can index it
  const jc_geom* gp;
  long cb, ob;
  if constexpr (GS::ragged) {
    __shared__ jc_geom frame_geom;
    __shared__ long frame_cb;
    __shared__ int frame_ok;
    if (t == 0) frame_ok = gs.frame(f, frame_geom, &frame_cb, &ob);
    __syncthreads();
    if (!frame_ok) return;                                                 // uniform
    gp = &frame_geom;
    cb = frame_cb;
  } else {
    typename GS::store none;
    gs.frame(f, none, &cb, &ob);
    gp = &gs.geom(none);
  }
  const jc_geom& g = *gp;
  const int32_t* m = meta + f * width;
  if (jc_segment_count(m, width, maxseg) != 1) return;                     // uniform: jpeg_entropy_kernel's frame
  int s0, s1, m0, m1;
  if (!jc_segment_range(m, width, maxseg, data_len, 0, g, &s0, &s1, &m0, &m1)) return;
  int32_t* tab = split_lds;                                                // quantisers and Huffman tables
  int32_t* ex = tab + JM_SEG;                                              // [L][2] exit states
  uint32_t* ps = reinterpret_cast<uint32_t*>(ex + 2 * L);                  // [L][4] blocks, DC sums
  int32_t* carry = reinterpret_cast<int32_t*>(ps + 4 * L);                 // state (2), blocks, DC predictors (3)
  for (int i = t; i < JM_SEG; i += L) tab[i] = m[i];
  if (t == 0) {
    carry[0] = s0;
    carry[1] = carry[2] = carry[3] = carry[4] = carry[5] = 0;
  }
  __syncthreads();
  const uint32_t total = (uint32_t)((long)(m1 - m0) * g.mcu_blocks);
  int16_t* dst = coef + cb * 64;
  int st = 0;
  split_windows(data, s0, s1, chunk_bytes, tab, g, total, ex, ps, carry,
                [&](long, int cend, const jc_state& in, uint32_t block, const uint32_t* sums) {
                  const int dc[3] = {(int16_t)sums[0], (int16_t)sums[1], (int16_t)sums[2]};
                  st |= jc_chunk_write(data, s1, cend, chunk_bytes, tab, g, in, (long)block, dc, m0, m1, dst);
                });
  if (st) atomicOr(&status[f], st);
}

size_t split_lds_bytes(int lanes) { return ((size_t)JM_SEG + 6 * (size_t)lanes + 8) * 4; }

template <class GS>
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, long n, GS gs,
                                                        uint8_t* __restrict__ planes) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  typename GS::store gst;
  long cb;
  int blk;
  if (!gs.block(id, gst, &cb, &blk)) return;
  const jc_geom& g = gs.geom(gst);
  __attribute__((aligned(16))) int16_t in[64];
  const uint4* src = reinterpret_cast<const uint4*>(coef + (cb + blk) * 64);   // 128 bytes per block, 16-byte aligned
#pragma unroll
  for (int i = 0; i < 8; ++i) reinterpret_cast<uint4*>(in)[i] = src[i];
  long stride;
  const long at = jc_block_samples(g, blk, &stride);
  jc_idct_block(in, planes + cb * 64 + at, stride);
}

// vec: W % 16 == 0 and the frame's first byte 16-byte aligned, so every group of 16 pixels is three aligned 16-byte
// stores.  One geometry: the host decides for the call (`aligned`).  Ragged: `aligned` says that `out` itself is,
// and every frame answers for its own width and offset.
template <class GS>
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, long n, int groups,
                                                          GS gs, int aligned, uint8_t* __restrict__ out) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  typename GS::store gst;
  typename GS::box box;
  long cb, ob;
  int y, xg;
  if (!gs.group(id, groups, gst, box, &cb, &ob, &y, &xg)) return;
  const jc_geom& g = gs.geom(gst);
  const uint8_t* p = planes + cb * 64;
  const int width = gs.width(gst, box);                                    // of an output row: g.W, or the box's
  uint8_t* o = out + ob + ((long)y * width + (long)xg * 16) * 3;
  const int x0 = xg * 16;
  const int fx = gs.x0(box) + x0, fy = gs.y0(box) + y;                     // the group's first pixel in the frame
  if (aligned && gs.vec_ok(width, ob)) {
    __attribute__((aligned(16))) uint8_t px[48];
#pragma unroll
    for (int i = 0; i < 16; ++i) jc_pixel(p, g, fx + i, fy, px + 3 * i);
#pragma unroll
    for (int i = 0; i < 3; ++i) reinterpret_cast<uint4*>(o)[i] = reinterpret_cast<const uint4*>(px)[i];
  } else {
    const int nx = width - x0 < 16 ? width - x0 : 16;
    for (int i = 0; i < nx; ++i) {
      uint8_t px[3];
      jc_pixel(p, g, fx + i, fy, px);
      o[3 * i] = px[0];
      o[3 * i + 1] = px[1];
      o[3 * i + 2] = px[2];
    }
  }
}

bool geometry_ok(int H, int W, int ncomp, int hs, int vs) {
  return jc_geometry_ok(H, W, ncomp, hs, vs, JPEG_MAX_SIDE);
}

// ---- the host side: what every entry point checks and launches alike ------------------------------------------------

// The quantisers and Huffman tables of a descriptor (words JM_QUANT .. JM_SEG of m) are in the kernels' ranges.  Run per
// frame of every call; a function of its own on a cache line's start, since where these loops fall in the library
// otherwise moves a call's host time by a third (0.16 against 0.11 ms at 776 frames, the same object code).
__attribute__((noinline, aligned(64))) bool tables_ok(const int32_t* m, int ncomp) {
  for (int i = 0; i < 64 * ncomp; ++i)
    if (m[JM_QUANT + i] < 0 || m[JM_QUANT + i] > 255) return false;
  for (int t = 0; t < 6; ++t) {
    const int32_t* h = m + JM_HUFF + t * JM_HUFF_WORDS;
    for (int l = 0; l < 16; ++l)
      if (h[l] < 0 || h[l] > 65536 || (l && h[l] < h[l - 1]) || h[16 + l] < -65536 || h[16 + l] > 255) return false;
  }
  return true;
}

// the first bytes of a frame's restart segments do not go back and stay inside its `len` bytes
bool offsets_ok(const int32_t* seg, long nseg, long len) {
  long last = 0;
  for (long s = 0; s < nseg; ++s) {
    if (seg[s] < last || seg[s] > len) return false;
    last = seg[s];
  }
  return true;
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
    if (!offsets_ok(m + JM_SEG, nseg, len) || !tables_ok(m, g.ncomp)) return false;
    if (nseg > most) most = (int)nseg;
  }
  *maxseg = most;
  return true;
}

// Frame f of a table-driven call (t: its row of the geometry table, g: its geometry, obytes: its output): the storage
// is in frame order, no overlap, inside the buffers, an output frame 16-byte aligned, cend / oend the end of the frames
// so far; and the prefixes of blocks and of row groups (prefix_host, F + 1 words each) grow by `blocks` and `groups`.
bool frame_storage_ok(const int64_t* t, const jc_geom& g, long obytes, long blocks, long groups,
                      const int64_t* prefix_host, int F, int f, long coef_blocks, long out_bytes, long& cend,
                      long& oend) {
  const int64_t* pblocks = prefix_host + f;
  const int64_t* prows = prefix_host + F + 1 + f;
  const long cb = t[JR_CBLOCK], ob = t[JR_OBYTE];
  if (cb < cend || cb > coef_blocks - g.nblocks) return false;
  if (ob < oend || (ob & 15) || ob > out_bytes - obytes) return false;
  cend = cb + g.nblocks;
  oend = ob + obytes;
  return pblocks[1] - pblocks[0] == blocks && prows[1] - prows[0] == groups;
}

// Who decodes what.  chunks(f): the chunks of frame f if it is ONE segment, which a workgroup of the relaxation
// kernels takes, else 0.  -> how many such frames, and the chunks of the longest.
struct split_plan { long single = 0, most_chunks = 1; };

template <class Chunks>
split_plan plan_split(long f0, long f1, Chunks chunks) {
  split_plan p;
  for (long f = f0; f < f1; ++f) {
    const long n = chunks(f);
    if (n < 1) continue;
    ++p.single;
    if (n > p.most_chunks) p.most_chunks = n;
  }
  return p;
}

// a relaxation workgroup has a lane per chunk of the call's longest frame, in whole waves, up to 1024
int split_lanes(long most_chunks) { return most_chunks > 1024 ? 1024 : (int)((most_chunks + 63) / 64 * 64); }

// no launch of a call may need more workgroups than a grid has
bool grid_ok(long lanes1, int per1, long lanes2, long lanes3) {
  const long limit = 0x7fffffffL;
  return lanes1 / per1 < limit && lanes2 / 256 < limit && lanes3 / 256 < limit;
}

// What the stages of one call work on: the frames' coefficient blocks are [first, cend) of coefs, lanes2 / lanes3 the
// lanes of the inverse DCT and of the colour stage, groups / aligned what jpeg_colour_kernel takes.
struct stage_args {
  int F, stages;
  int16_t* coefs;
  uint8_t* planes;
  uint8_t* out;
  int32_t* status;
  long first, cend, lanes2, lanes3;
  int groups, aligned;
  hipStream_t s;
};

// The stages over the geometry source GS; entropy() launches the call's own entropy kernels onto zeroed coefficients
// and status words and returns 0 or an error.
template <class GS, class Entropy>
int run_stages(const GS& gs, const stage_args& a, Entropy entropy) {
  if (a.stages & 1) {
    COCLR_RETURN_IF(hipMemsetAsync(a.coefs + a.first * 64, 0, (size_t)(a.cend - a.first) * 128, a.s));
    COCLR_RETURN_IF(hipMemsetAsync(a.status, 0, (size_t)a.F * 4, a.s));
    const int e = entropy();
    if (e) return e;
  }
  if (a.stages & 2) {
    hipLaunchKernelGGL(jpeg_idct_kernel<GS>, dim3(cdiv(a.lanes2, 256)), dim3(256), 0, a.s, a.coefs, a.lanes2, gs,
                       a.planes);
    COCLR_LAUNCH_CHECK();
  }
  if (a.stages & 4) {
    hipLaunchKernelGGL(jpeg_colour_kernel<GS>, dim3(cdiv(a.lanes3, 256)), dim3(256), 0, a.s, a.planes, a.lanes3,
                       a.groups, gs, a.aligned, a.out);
    COCLR_LAUNCH_CHECK();
  }
  return 0;
}

// The entropy stage of a call on descriptors: frames of one segment go to the split kernel when chunk_bytes asked for
// it (plan), all others to a lane per restart segment.
template <class GS>
int launch_entropy(const GS& gs, const uint8_t* data, int64_t data_len, const int32_t* meta, int width, int F,
                   int maxseg, const split_plan& plan, int chunk_bytes, int16_t* coefs, int32_t* status,
                   hipStream_t s) {
  if (plan.single < F) {
    hipLaunchKernelGGL(jpeg_entropy_kernel<GS>, dim3(cdiv((long)F * maxseg, 64)), dim3(64), 0, s, data, (int)data_len,
                       meta, width, F, maxseg, plan.single > 0 ? 1 : 0, gs, coefs, status);
    COCLR_LAUNCH_CHECK();
  }
  if (plan.single > 0) {
    const int lanes = split_lanes(plan.most_chunks);
    hipLaunchKernelGGL(jpeg_entropy_split_kernel<GS>, dim3(F), dim3(lanes), split_lds_bytes(lanes), s, data,
                       (int)data_len, meta, width, maxseg, chunk_bytes, gs, coefs, status);
    COCLR_LAUNCH_CHECK();
  }
  return 0;
}

// The tail of both calls on descriptors: who decodes what (geom_of(f): frame f's geometry, on the host; maxseg is the
// call's, as the kernels clamp with it), then the stages.
template <class GS, class GeomOf>
int decode_descriptors(const GS& gs, const stage_args& a, const uint8_t* data, int64_t data_len, const int32_t* meta,
                       const int32_t* meta_host, int width, int maxseg, int chunk_bytes, GeomOf geom_of) {
  if (!grid_ok((long)a.F * maxseg, 64, a.lanes2, a.lanes3)) return COCLR_EINVAL;
  split_plan plan;
  if (chunk_bytes)
    plan = plan_split(0, a.F, [&](long f) -> long {
      const int32_t* m = meta_host + f * width;
      int s0, s1, m0, m1;
      if (jc_segment_count(m, width, maxseg) != 1 ||
          !jc_segment_range(m, width, maxseg, (int)data_len, 0, geom_of(f), &s0, &s1, &m0, &m1))
        return 0;
      return jc_chunk_count(s0, s1, chunk_bytes);
    });
  return run_stages(gs, a, [&] {
    return launch_entropy(gs, data, data_len, meta, width, a.F, maxseg, plan, chunk_bytes, a.coefs, a.status, a.s);
  });
}

// what the two calls on descriptors ask of their common arguments
bool descriptor_args_ok(const uint8_t* data, int64_t data_len, const int32_t* meta, const int32_t* meta_host, int F,
                        int width, int stages, const int16_t* coefs, const uint8_t* planes, const uint8_t* out,
                        const int32_t* status, int chunk_bytes) {
  if (!data || !meta || !meta_host || !coefs || !planes || !out || !status) return false;
  if (F < 1 || width <= JM_SEG || data_len < 0 || data_len > 0x7fffffff || stages < 1 || stages > 7) return false;
  if (((uintptr_t)coefs & 15) || ((uintptr_t)meta & 3)) return false;
  return chunk_bytes == 0 || (chunk_bytes >= 8 && chunk_bytes <= 65536);
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

namespace {

// coclr_jpeg_decode and coclr_jpeg_decode_split: one geometry, frame f at f times the per-frame sizes.  `planes` and
// `out` may lie anywhere; whether the colour stage stores 16 bytes at a time is decided here, for the call.
int jpeg_decode_impl(const uint8_t* data, int64_t data_len, const int32_t* meta, const int32_t* meta_host, int F,
                     int width, int H, int W, int ncomp, int hs, int vs, int stages, int16_t* coefs, uint8_t* planes,
                     uint8_t* out, int32_t* status, int chunk_bytes, void* stream) {
  if (!descriptor_args_ok(data, data_len, meta, meta_host, F, width, stages, coefs, planes, out, status, chunk_bytes))
    return COCLR_EINVAL;
  if (!geometry_ok(H, W, ncomp, hs, vs)) return COCLR_EINVAL;
  jc_geom g;
  jc_geom_init(g, H, W, ncomp, hs, vs);
  int maxseg = 1;
  if (!meta_ok(meta_host, F, width, data_len, g, &maxseg)) return COCLR_EINVAL;
  const int groups = (W + 15) / 16;
  const stage_args a = {F, stages, coefs, planes, out, status, 0, (long)F * g.nblocks, (long)F * g.nblocks,
                        (long)F * H * groups, groups, W % 16 == 0 && ((uintptr_t)out & 15) == 0, (hipStream_t)stream};
  return decode_descriptors(one_geom{g}, a, data, data_len, meta, meta_host, width, maxseg, chunk_bytes,
                            [&](long) -> const jc_geom& { return g; });
}

}  // namespace

extern "C" int coclr_jpeg_decode(const uint8_t* data, int64_t data_len, const int32_t* meta, const int32_t* meta_host,
                                 int F, int width, int H, int W, int ncomp, int hs, int vs, int stages, int16_t* coefs,
                                 uint8_t* planes, uint8_t* out, int32_t* status, void* stream) {
  return jpeg_decode_impl(data, data_len, meta, meta_host, F, width, H, W, ncomp, hs, vs, stages, coefs, planes, out,
                          status, 0, stream);
}

extern "C" int coclr_jpeg_decode_split(const uint8_t* data, int64_t data_len, const int32_t* meta,
                                       const int32_t* meta_host, int F, int width, int H, int W, int ncomp, int hs,
                                       int vs, int stages, int16_t* coefs, uint8_t* planes, uint8_t* out,
                                       int32_t* status, int chunk_bytes, void* stream) {
  return jpeg_decode_impl(data, data_len, meta, meta_host, F, width, H, W, ncomp, hs, vs, stages, coefs, planes, out,
                          status, chunk_bytes, stream);
}

// Frames of differing geometry in one call: jpeg_decode_impl with the geometry, the first coefficient block and the
// first output byte per frame (jpeg_core.h: JR_*), from tables that are checked on their host copies first; the
// buffers must be 16-byte aligned.
extern "C" int coclr_jpeg_decode_ragged(const uint8_t* data, int64_t data_len, const int32_t* meta,
                                        const int32_t* meta_host, int F, int width, const int64_t* geom,
                                        const int64_t* geom_host, const int64_t* prefix, const int64_t* prefix_host,
                                        int stages, int16_t* coefs, uint8_t* planes, int64_t coef_blocks, uint8_t* out,
                                        int64_t out_bytes, int32_t* status, int chunk_bytes, void* stream) {
  if (!descriptor_args_ok(data, data_len, meta, meta_host, F, width, stages, coefs, planes, out, status, chunk_bytes))
    return COCLR_EINVAL;
  if (!geom || !geom_host || !prefix || !prefix_host || coef_blocks < 1 || out_bytes < 1) return COCLR_EINVAL;
  if (((uintptr_t)planes & 15) || ((uintptr_t)out & 15) || ((uintptr_t)geom & 7) || ((uintptr_t)prefix & 7))
    return COCLR_EINVAL;
  if (prefix_host[0] != 0 || prefix_host[F + 1] != 0) return COCLR_EINVAL;
  const auto geom_of = [&](long f) {
    const int64_t* t = geom_host + f * JR_FIELDS;
    jc_geom g;
    jc_geom_init(g, (int)t[JR_H], (int)t[JR_W], (int)t[JR_NCOMP], (int)t[JR_HS], (int)t[JR_VS]);
    return g;
  };
  int maxseg = 1;
  long cend = 0, oend = 0;
  for (int f = 0; f < F; ++f) {
    const int64_t* t = geom_host + (long)f * JR_FIELDS;
    if (!jc_geometry_ok(t[JR_H], t[JR_W], t[JR_NCOMP], t[JR_HS], t[JR_VS], JPEG_MAX_SIDE)) return COCLR_EINVAL;
    const jc_geom g = geom_of(f);
    if (!frame_storage_ok(t, g, (long)g.H * g.W * 3, g.nblocks, jc_row_groups(g), prefix_host, F, f, coef_blocks,
                          out_bytes, cend, oend))
      return COCLR_EINVAL;
    int segs = 1;
    if (!meta_ok(meta_host + (long)f * width, 1, width, data_len, g, &segs)) return COCLR_EINVAL;
    if (segs > maxseg) maxseg = segs;
  }
  const stage_args a = {F, stages, coefs, planes, out, status, (long)geom_host[JR_CBLOCK], cend, (long)prefix_host[F],
                        (long)prefix_host[2 * F + 1], 0, 1, (hipStream_t)stream};
  return decode_descriptors(ragged_geom{geom, nullptr, prefix, prefix + F + 1, F, coef_blocks, out_bytes}, a, data,
                            data_len, meta, meta_host, width, maxseg, chunk_bytes, geom_of);
}

// ---- frames of a device-resident store, decoded by index ------------------------------------------------------------
namespace {

struct store_view {          // the device side of a coclr_jpeg_store
  const uint8_t* data;
  long data_bytes;
  const int64_t* frames;
  long nframes;
  const int32_t* tables;
  long table_sets;
  const int32_t* segs;
  long nsegs;
  uint32_t* rows;
  long nrows;
  int chunk_bytes;
};

// One workgroup per frame f0 + blockIdx.x of ONE segment (the others return at once): split_windows, every chunk's
// true state stored (jc_row_pack) where jpeg_entropy_split_kernel decodes from it.  Once only zero bits are left
// every later chunk's row says so.  Dynamic LDS as there (split_lds_bytes); every barrier is on a workgroup-uniform
// path.
__global__ __launch_bounds__(1024) void jpeg_store_index_kernel(store_view sv, long f0) {
  extern __shared__ int32_t index_lds[];
  __shared__ jc_geom g;
  const int t = threadIdx.x, L = blockDim.x;
  const long f = f0 + blockIdx.x;
  if (f < 0 || f >= sv.nframes) return;                                    // uniform
  jc_store_frame fr;
  jc_store_frame_get(sv.frames + f * JS_FIELDS, sv.data, sv.data_bytes, sv.tables, sv.table_sets, fr);
  if (fr.nseg != 1 || !jc_geometry_ok(fr.H, fr.W, fr.ncomp, fr.hs, fr.vs, JPEG_MAX_SIDE)) return;   // uniform
  const int chunk_bytes = sv.chunk_bytes;
  const int s1 = fr.len;
  const long nchunks = jc_chunk_count(0, s1, chunk_bytes);
  if (fr.row < 0 || fr.row > sv.nrows - nchunks) return;                    // uniform
  int32_t* tab = index_lds;                                                // quantisers and Huffman tables
  int32_t* ex = tab + JM_SEG;                                              // [L][2] exit states
  uint32_t* ps = reinterpret_cast<uint32_t*>(ex + 2 * L);                  // [L][4] blocks, DC sums
  int32_t* carry = reinterpret_cast<int32_t*>(ps + 4 * L);                 // state (2), blocks, DC predictors (3)
  for (int i = JM_QUANT + t; i < JM_SEG; i += L) tab[i] = fr.meta[i];
  if (t == 0) {
    jc_geom_init(g, (int)fr.H, (int)fr.W, (int)fr.ncomp, (int)fr.hs, (int)fr.vs);
    carry[0] = carry[1] = carry[2] = carry[3] = carry[4] = carry[5] = 0;
  }
  __syncthreads();
  const uint32_t total = (uint32_t)((long)g.mcux * g.mcuy * g.mcu_blocks);
  uint32_t* rows = sv.rows + fr.row * JS_ROW_WORDS;
  const auto store_row = [&](long chunk, const jc_state& in, long start, uint32_t block, const uint32_t* dc) {
    uint32_t row[JS_ROW_WORDS];
    jc_row_pack(row, in, start, block, dc);
    *reinterpret_cast<uint4*>(rows + chunk * JS_ROW_WORDS) = make_uint4(row[0], row[1], row[2], row[3]);
  };
  const long reached = split_windows(fr.bytes, 0, s1, chunk_bytes, tab, g, total, ex, ps, carry,
                                     [&](long chunk, int, const jc_state& in, uint32_t block, const uint32_t* dc) {
                                       store_row(chunk, in, jc_chunk_start(s1, chunk_bytes, chunk), block, dc);
                                     });
  const uint32_t none[3] = {0, 0, 0};
  for (long i = reached + t; i < nchunks; i += L) store_row(i, jc_state_past(), 0, total, none);   // past the real bits
}

// The entropy stage of coclr_jpeg_decode_store, one pass: lane id is chunk or restart segment `local` of call frame f
// (binary search in the lane prefix), which is store frame sel[f].  The geometry and the coefficient blocks are the
// call's (gs, checked against coef_blocks); bytes, tables and rows are the store's, clamped.
// GS = window_geom (coclr_jpeg_decode_store_window): only MCUs [first, last) of the frame, the linear range of the
// window's MCU rectangle, are wanted.  A chunk's lane also loads the NEXT row's block count (a past row, or none: the
// frame's), returns when the blocks it touches miss the range (jc_window_skips_blocks), and else decodes up to `last`;
// a segment's lane returns when its MCUs miss the range.  No lane depends on another, so the lanes that run write what
// they write in a full decode.
template <class GS>
__global__ __launch_bounds__(256) void jpeg_entropy_store_kernel(store_view sv, const int64_t* __restrict__ sel,
                                                                 const int64_t* __restrict__ lanes, long n, GS gs,
                                                                 int16_t* __restrict__ coef,
                                                                 int32_t* __restrict__ status) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const long f = jc_find_frame(lanes, gs.F, id);
  const long local = id - lanes[f];
  jc_geom g;
  typename GS::box box;
  long cb, ob;
  if (local < 0) return;
  if (!gs.frame(f, g, box, &cb, &ob)) return;
  long sf = sel[f];
  sf = sf < 0 || sf >= sv.nframes ? 0 : sf;
  jc_store_frame fr;
  jc_store_frame_get(sv.frames + sf * JS_FIELDS, sv.data, sv.data_bytes, sv.tables, sv.table_sets, fr);
  int16_t* dst = coef + cb * 64;
  int st = 0;
  if (fr.nseg == 1) {
    const long at = fr.row + local;
    if (local >= jc_chunk_count(0, fr.len, sv.chunk_bytes) || fr.row < 0 || at >= sv.nrows) return;
    const uint4 w = *reinterpret_cast<const uint4*>(sv.rows + at * JS_ROW_WORDS);
    const uint32_t row[JS_ROW_WORDS] = {w.x, w.y, w.z, w.w};
    long block;
    int dc[3];
    const jc_state in = jc_row_unpack(row, jc_chunk_start(fr.len, sv.chunk_bytes, local), fr.len, g, &block, dc);
    int last = g.mcux * g.mcuy;
    if constexpr (GS::windowed) {
      long next = (long)last * g.mcu_blocks;
      if (local + 1 < jc_chunk_count(0, fr.len, sv.chunk_bytes) && at + 1 < sv.nrows) {
        const uint2 nw = *reinterpret_cast<const uint2*>(sv.rows + (at + 1) * JS_ROW_WORDS);
        if (!(nw.x >> 31)) next = (long)nw.y;
      }
      if (jc_window_skips_blocks(g, box, block, next)) return;
      last = (int)jc_window_last(g, box);
    }
    st = jc_chunk_write(fr.bytes, fr.len, jc_chunk_end(0, fr.len, sv.chunk_bytes, local), sv.chunk_bytes, fr.meta, g,
                        in, block, dc, 0, last, dst);
  } else {
    int s0, s1, m0, m1;
    if (!jc_store_segment(fr, sv.segs, sv.nsegs, local, g, &s0, &s1, &m0, &m1)) return;
    if constexpr (GS::windowed)
      if (jc_window_skips_mcus(g, box, m0, m1)) return;
    st = jc_decode_segment(fr.bytes, s0, s1, fr.meta, g, m0, m1, dst);
  }
  if (st) atomicOr(&status[f], st);
}

bool store_ok(const coclr_jpeg_store* st) {
  if (!st || !st->data || !st->frames || !st->frames_host || !st->tables || !st->tables_host || !st->rows)
    return false;
  if (st->data_bytes < 0 || st->nframes < 1 || st->table_sets < 1 || st->nsegs < 0 || st->nrows < 1) return false;
  if (st->nsegs > 0 && (!st->segs || !st->segs_host)) return false;
  if (st->chunk_bytes < 8 || st->chunk_bytes > 65536) return false;
  return !(((uintptr_t)st->frames & 7) || ((uintptr_t)st->tables & 3) || ((uintptr_t)st->segs & 3) ||
           ((uintptr_t)st->rows & 15));
}

store_view store_device(const coclr_jpeg_store* st) {
  return {st->data, st->data_bytes, st->frames, st->nframes, st->tables, st->table_sets,
          st->segs,  st->nsegs,     st->rows,   st->nrows,   st->chunk_bytes};
}

// the host copy of store frame f: its buffers' bounds; with `deep` also what meta_ok checks of a descriptor
bool store_frame_ok(const coclr_jpeg_store* st, long f, bool deep, jc_store_frame& fr, jc_geom& g) {
  const int64_t* rec = st->frames_host + f * JS_FIELDS;
  const int64_t base = rec[JS_BASE], len = rec[JS_LEN], nseg = rec[JS_NSEG], ri = rec[JS_RI];
  if (base < 0 || len < 0 || len > 0x7fffffff || base > st->data_bytes - len) return false;
  if (rec[JS_TSET] < 0 || rec[JS_TSET] >= st->table_sets || nseg < 1 || nseg > 0x7fffffff || ri < 0) return false;
  jc_store_frame_get(rec, st->data, st->data_bytes, st->tables_host, st->table_sets, fr);
  if (!jc_geometry_ok(fr.H, fr.W, fr.ncomp, fr.hs, fr.vs, JPEG_MAX_SIDE)) return false;
  jc_geom_init(g, (int)fr.H, (int)fr.W, (int)fr.ncomp, (int)fr.hs, (int)fr.vs);
  const long total = (long)g.mcux * g.mcuy;
  if (nseg != (ri == 0 ? 1 : (total + ri - 1) / ri)) return false;
  if (nseg == 1) {
    if (fr.row < 0 || fr.row > st->nrows - jc_chunk_count(0, fr.len, st->chunk_bytes)) return false;
  } else if (fr.seg < 0 || fr.seg > st->nsegs - nseg) {
    return false;
  }
  if (!deep) return true;
  return (nseg == 1 || offsets_ok(st->segs_host + fr.seg, nseg, len)) && tables_ok(fr.meta, g.ncomp);
}

}  // namespace

extern "C" int coclr_jpeg_store_index(const coclr_jpeg_store* st, int64_t f0, int64_t f1, void* stream) {
  if (!store_ok(st) || f0 < 0 || f1 <= f0 || f1 > st->nframes || f1 - f0 >= 0x7fffffffL) return COCLR_EINVAL;
  bool ok = true;
  const split_plan plan = plan_split(f0, f1, [&](long f) -> long {
    jc_store_frame fr;
    jc_geom g;
    ok = ok && store_frame_ok(st, f, true, fr, g);
    return ok && fr.nseg == 1 ? jc_chunk_count(0, fr.len, st->chunk_bytes) : 0;
  });
  if (!ok) return COCLR_EINVAL;
  if (!plan.single) return 0;
  const int lanes = split_lanes(plan.most_chunks);
  hipLaunchKernelGGL(jpeg_store_index_kernel, dim3((unsigned)(f1 - f0)), dim3(lanes), split_lds_bytes(lanes),
                     (hipStream_t)stream, store_device(st), (long)f0);
  COCLR_LAUNCH_CHECK();
  return 0;
}

namespace {

// coclr_jpeg_decode_store (window == nullptr) and coclr_jpeg_decode_store_window: everything is checked on the host
// copies first.  With a window table the output frame is the box (3 * w * h bytes) and the block and row-group
// prefixes count the box's MCU rectangle and rows; the MCU rectangle is derived here, from the box and the store's
// host record, never taken from the caller.
int jpeg_decode_store_impl(const coclr_jpeg_store* st, const int64_t* sel, const int64_t* sel_host, int F,
                           const int64_t* geom, const int64_t* geom_host, const int64_t* window,
                           const int64_t* window_host, const int64_t* prefix, const int64_t* prefix_host, int stages,
                           int16_t* coefs, uint8_t* planes, int64_t coef_blocks, uint8_t* out, int64_t out_bytes,
                           int32_t* status, void* stream) {
  if (!store_ok(st) || !sel || !sel_host || !geom || !geom_host || !prefix || !prefix_host || !coefs || !planes ||
      !out || !status)
    return COCLR_EINVAL;
  if (F < 1 || stages < 1 || stages > 7 || coef_blocks < 1 || out_bytes < 1) return COCLR_EINVAL;
  if (((uintptr_t)coefs & 15) || ((uintptr_t)planes & 15) || ((uintptr_t)out & 15) || ((uintptr_t)sel & 7) ||
      ((uintptr_t)geom & 7) || ((uintptr_t)prefix & 7) || ((uintptr_t)window & 7))
    return COCLR_EINVAL;
  const int64_t* pchunks = prefix_host + 2 * (F + 1);
  if (prefix_host[0] != 0 || prefix_host[F + 1] != 0 || pchunks[0] != 0) return COCLR_EINVAL;
  long cend = 0, oend = 0;
  for (int f = 0; f < F; ++f) {
    const int64_t* t = geom_host + (long)f * JR_FIELDS;
    if (sel_host[f] < 0 || sel_host[f] >= st->nframes) return COCLR_EINVAL;
    jc_store_frame fr;
    jc_geom g;
    if (!store_frame_ok(st, sel_host[f], false, fr, g)) return COCLR_EINVAL;
    if (t[JR_H] != fr.H || t[JR_W] != fr.W || t[JR_NCOMP] != fr.ncomp || t[JR_HS] != fr.hs || t[JR_VS] != fr.vs)
      return COCLR_EINVAL;
    long obytes = (long)g.H * g.W * 3, nblocks = g.nblocks, ngroups = jc_row_groups(g);
    if (window_host) {
      const int64_t* b = window_host + (long)f * JW_FIELDS;
      jc_window w;
      if (!jc_window_init(g, b[JW_X0], b[JW_Y0], b[JW_W], b[JW_H], w)) return COCLR_EINVAL;
      obytes = (long)w.w * w.h * 3;
      nblocks = jc_window_blocks(g, w);
      ngroups = jc_window_row_groups(w);
    }
    if (!frame_storage_ok(t, g, obytes, nblocks, ngroups, prefix_host, F, f, coef_blocks, out_bytes, cend, oend))
      return COCLR_EINVAL;
    if (pchunks[f + 1] - pchunks[f] != jc_store_lanes(fr.len, fr.nseg, st->chunk_bytes)) return COCLR_EINVAL;
  }
  const stage_args a = {F, stages, coefs, planes, out, status, (long)geom_host[JR_CBLOCK], cend, (long)prefix_host[F],
                        (long)prefix_host[2 * F + 1], 0, 1, (hipStream_t)stream};
  const long lanes1 = pchunks[F];
  if (!grid_ok(lanes1, 256, a.lanes2, a.lanes3)) return COCLR_EINVAL;
  // one pass: a lane per chunk or restart segment of any frame of the call, from the store's rows
  const auto stages_over = [&](const auto& gs) {
    typedef std::decay_t<decltype(gs)> GS;
    return run_stages(gs, a, [&] {
      hipLaunchKernelGGL(jpeg_entropy_store_kernel<GS>, dim3(cdiv(lanes1, 256)), dim3(256), 0, a.s, store_device(st),
                         sel, prefix + 2 * (F + 1), lanes1, gs, coefs, status);
      COCLR_LAUNCH_CHECK();
      return 0;
    });
  };
  if (window_host) return stages_over(window_geom{geom, window, prefix, prefix + F + 1, F, coef_blocks, out_bytes});
  return stages_over(ragged_geom{geom, nullptr, prefix, prefix + F + 1, F, coef_blocks, out_bytes});
}

}  // namespace

extern "C" int coclr_jpeg_decode_store(const coclr_jpeg_store* st, const int64_t* sel, const int64_t* sel_host, int F,
                                       const int64_t* geom, const int64_t* geom_host, const int64_t* prefix,
                                       const int64_t* prefix_host, int stages, int16_t* coefs, uint8_t* planes,
                                       int64_t coef_blocks, uint8_t* out, int64_t out_bytes, int32_t* status,
                                       void* stream) {
  return jpeg_decode_store_impl(st, sel, sel_host, F, geom, geom_host, nullptr, nullptr, prefix, prefix_host, stages,
                                coefs, planes, coef_blocks, out, out_bytes, status, stream);
}

extern "C" int coclr_jpeg_decode_store_window(const coclr_jpeg_store* st, const int64_t* sel, const int64_t* sel_host,
                                              int F, const int64_t* geom, const int64_t* geom_host,
                                              const int64_t* window, const int64_t* window_host, const int64_t* prefix,
                                              const int64_t* prefix_host, int stages, int16_t* coefs, uint8_t* planes,
                                              int64_t coef_blocks, uint8_t* out, int64_t out_bytes, int32_t* status,
                                              void* stream) {
  if (!window || !window_host) return COCLR_EINVAL;
  return jpeg_decode_store_impl(st, sel, sel_host, F, geom, geom_host, window, window_host, prefix, prefix_host, stages,
                                coefs, planes, coef_blocks, out, out_bytes, status, stream);
}

// ---- a selection of store frames copied to a device arena -----------------------------------------------------------
namespace {

// Where a gather's lanes read from.  one_source: the call's single source, in the arguments (coclr_jpeg_store_gather).
// shard_sources: a by-value table of up to JG_MAX_SHARDS sources and the device column that names each plan row's
// (coclr_jpeg_store_gather_shards); a row whose shard lies outside the table copies nothing.
// find(): jpeg_core.h's lane arithmetic held against the lane's own source and the arena -> that source, or null.
struct jg_source {
  const uint4* data;
  long words;                  // the 16-byte words its bytes touch
  const uint4* rows;
  long nrows;
};

struct one_source {
  jg_source s;
  __device__ const jg_source* find(const int64_t* plan, long m, long id, long arena_words, long arena_nrows,
                                   bool* rows, int64_t* src, int64_t* dst) const {
    return jc_gather_lane(plan, m, id, s.words, s.nrows, arena_words, arena_nrows, rows, src, dst) ? &s : nullptr;
  }
};

struct shard_sources {
  jg_source s[JG_MAX_SHARDS];
  const int64_t* shard;        // int64 [m], DEVICE
  long n;
  __device__ const jg_source* find(const int64_t* plan, long m, long id, long arena_words, long arena_nrows,
                                   bool* rows, int64_t* src, int64_t* dst) const {
    int64_t which;
    if (!jc_gather_lane_from(plan, shard, m, id, s, n, arena_words, arena_nrows, &which, rows, src, dst))
      return nullptr;
    return &s[which];
  }
};

// A lane per 16-byte word: the words of every distinct frame's hull, then its rows (jpeg_core.h: jc_gather_lane_from).
// A source may be pinned host memory or a peer's memory: one 16-byte load and one 16-byte store per lane, no byte
// path.  The plan (and the shard column) is the device copy; the sizes are the host's, by value, and no word outside
// them is touched whatever the device data holds.
template <class SRC, class... ARGS>    // ARGS: what SRC is made of, as the kernel's leading arguments
__global__ __launch_bounds__(256) void jpeg_store_gather_kernel(ARGS... source, const int64_t* __restrict__ plan,
                                                                long m, long lanes, uint4* __restrict__ arena,
                                                                long arena_words, uint4* __restrict__ arena_rows,
                                                                long arena_nrows) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= lanes) return;
  const SRC at{source...};
  bool rows;
  int64_t src, dst;
  const jg_source* s = at.find(plan, m, id, arena_words, arena_nrows, &rows, &src, &dst);
  if (!s) return;
  if (rows) arena_rows[dst] = s->rows[src];
  else arena[dst] = s->data[src];
}

// The address a kernel reads `bytes` bytes at `p` through: device memory, or host memory that is registered with the
// runtime (pinned) -- first and last byte alike.  Null for everything else (pageable or managed memory, no device),
// with the runtime's last error cleared: a kernel must never be launched on such a pointer.
const void* gather_source(const void* p, int64_t bytes) {
  const void* dev = nullptr;
  for (int end = 0; end < 2; ++end) {
    hipPointerAttribute_t at;
    const void* q = (const uint8_t*)p + (end ? bytes - 1 : 0);
    if (hipPointerGetAttributes(&at, q) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    if (at.isManaged || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeHost) || !at.devicePointer)
      return nullptr;
    if (at.type == hipMemoryTypeHost && !at.hostPointer) return nullptr;
    if (end) continue;
    // a host pointer's device address, by its distance from the host address the runtime answers with
    dev = at.type == hipMemoryTypeDevice
              ? p
              : (const uint8_t*)at.devicePointer + ((const uint8_t*)q - (const uint8_t*)at.hostPointer);
  }
  return dev;
}

}  // namespace

namespace {

// a shard of coclr_jpeg_store_gather_shards: store_ok for what a gather reads -- the bytes, the rows and the host
// tables -- and a shard may be EMPTY
bool gather_shard_ok(const coclr_jpeg_store* st) {
  if (!st || !st->data || !st->rows || !st->tables_host) return false;
  if (st->data_bytes < 1 || st->nframes < 0 || st->table_sets < 0 || st->nsegs < 0 || st->nrows < 1) return false;
  if ((st->nframes > 0 && !st->frames_host) || (st->nsegs > 0 && !st->segs_host)) return false;
  if (st->chunk_bytes < 8 || st->chunk_bytes > 65536) return false;
  return !(((uintptr_t)st->data & 15) || ((uintptr_t)st->rows & 15));
}

// The body of both gather entries.  `shard_host` null: the one source of coclr_jpeg_store_gather, every row's shard 0.
int gather_impl(const coclr_jpeg_store* const* shards, int nshards, const int64_t* plan, const int64_t* plan_host,
                const int64_t* shard, const int64_t* shard_host, int64_t m, const int64_t* slot_host,
                const int64_t* frames_host, int64_t n, uint8_t* arena, int64_t arena_bytes, uint32_t* arena_rows,
                int64_t arena_nrows, void* stream) {
  if (!plan || !plan_host || !slot_host || !frames_host || !arena || !arena_rows) return COCLR_EINVAL;
  if (m < 1 || n < m || n > 0x7fffffffL || arena_bytes < 1 || arena_nrows < 1) return COCLR_EINVAL;
  if (((uintptr_t)arena & 15) || ((uintptr_t)arena_rows & 15) || ((uintptr_t)plan & 7) || ((uintptr_t)shard & 7))
    return COCLR_EINVAL;
  int64_t end = 0, rows = 0, lanes = 0;
  for (int64_t j = 0; j < m; ++j) {
    const int64_t* p = plan_host + j * JG_FIELDS;
    if (shard_host && !jc_gather_order_ok(plan_host, shard_host, j, nshards)) return COCLR_EINVAL;
    const coclr_jpeg_store* st = shards[shard_host ? shard_host[j] : 0];
    const int64_t f = p[JG_FRAME];
    if (f < 0 || f >= st->nframes) return COCLR_EINVAL;
    jc_store_frame fr;
    jc_geom g;
    int64_t brings;
    const int64_t* rec = st->frames_host + f * JS_FIELDS;
    if (!store_frame_ok(st, f, false, fr, g) ||
        !jc_gather_frame_ok(rec, st->data_bytes, st->nrows, st->chunk_bytes, &brings))
      return COCLR_EINVAL;
    if (p[JG_SRC] != rec[JS_BASE] || p[JG_LEN] != rec[JS_LEN] || p[JG_SRCROW] != rec[JS_ROW] ||
        p[JG_NROWS] != brings || p[JG_LANE] != lanes)
      return COCLR_EINVAL;
    jc_span s;
    if (!jc_gather_span(p[JG_SRC], p[JG_LEN], p[JG_DST], s)) return COCLR_EINVAL;            // the congruence
    if (s.dst << 4 < end || s.dst << 4 > end + 15 || jc_gather_end(s) > arena_bytes)         // its neighbour; the
      return COCLR_EINVAL;                                                                   // arena: whole words
    if (p[JG_DSTROW] != rows || rows > arena_nrows - brings) return COCLR_EINVAL;
    end = jc_gather_end(s);
    rows += brings;
    lanes += s.words + brings;
  }
  for (int64_t i = 0; i < n; ++i) {
    const int64_t j = slot_host[i];
    if (j < 0 || j >= m) return COCLR_EINVAL;
    const int64_t* p = plan_host + j * JG_FIELDS;
    const coclr_jpeg_store* st = shards[shard_host ? shard_host[j] : 0];
    int64_t want[JS_FIELDS];
    jc_gather_rebase(st->frames_host + p[JG_FRAME] * JS_FIELDS, p[JG_DST], p[JG_DSTROW], want);
    for (int k = 0; k < JS_FIELDS; ++k)
      if (frames_host[i * JS_FIELDS + k] != want[k]) return COCLR_EINVAL;
  }
  if (lanes < 1) return 0;
  if (!grid_ok(lanes, 256, 0, 0)) return COCLR_EINVAL;
  shard_sources from = {};
  for (int k = 0; k < nshards; ++k) {                       // every source, whether or not a row reads it
    const coclr_jpeg_store* st = shards[k];
    const void* data = gather_source(st->data, st->data_bytes);
    const void* srows = gather_source(st->rows, st->nrows * JS_ROW_WORDS * 4);
    if (!data || !srows || ((uintptr_t)data & 15) || ((uintptr_t)srows & 15)) return COCLR_EINVAL;
    from.s[k] = {(const uint4*)data, (long)((st->data_bytes + 15) >> 4), (const uint4*)srows, (long)st->nrows};
  }
  const dim3 grid(cdiv(lanes, 256)), block(256);
  if (!shard_host) {
    const jg_source& one = from.s[0];
    hipLaunchKernelGGL((jpeg_store_gather_kernel<one_source, const uint4* __restrict__, long, const uint4* __restrict__,
                                                 long>),
                       grid, block, 0, (hipStream_t)stream, one.data, one.words, one.rows, one.nrows, plan, (long)m,
                       (long)lanes, (uint4*)arena, (long)(arena_bytes >> 4), (uint4*)arena_rows, (long)arena_nrows);
  } else {
    from.shard = shard;
    from.n = nshards;
    hipLaunchKernelGGL((jpeg_store_gather_kernel<shard_sources, shard_sources>), grid, block, 0, (hipStream_t)stream,
                       from, plan, (long)m, (long)lanes, (uint4*)arena, (long)(arena_bytes >> 4), (uint4*)arena_rows,
                       (long)arena_nrows);
  }
  COCLR_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int coclr_jpeg_store_gather(const coclr_jpeg_store* st, const int64_t* plan, const int64_t* plan_host,
                                       int64_t m, const int64_t* slot_host, const int64_t* frames_host, int64_t n,
                                       uint8_t* arena, int64_t arena_bytes, uint32_t* arena_rows, int64_t arena_nrows,
                                       void* stream) {
  if (!store_ok(st) || st->data_bytes < 1 || ((uintptr_t)st->data & 15)) return COCLR_EINVAL;
  return gather_impl(&st, 1, plan, plan_host, nullptr, nullptr, m, slot_host, frames_host, n, arena, arena_bytes,
                     arena_rows, arena_nrows, stream);
}

extern "C" int coclr_jpeg_store_gather_shards(const coclr_jpeg_store* const* shards, int nshards, const int64_t* plan,
                                              const int64_t* plan_host, const int64_t* shard,
                                              const int64_t* shard_host, int64_t m, const int64_t* slot_host,
                                              const int64_t* frames_host, int64_t n, uint8_t* arena,
                                              int64_t arena_bytes, uint32_t* arena_rows, int64_t arena_nrows,
                                              void* stream) {
  if (!shards || nshards < 1 || nshards > JG_MAX_SHARDS || !shard || !shard_host) return COCLR_EINVAL;
  for (int k = 0; k < nshards; ++k)
    if (!gather_shard_ok(shards[k]) || shards[k]->chunk_bytes != shards[0]->chunk_bytes) return COCLR_EINVAL;
  return gather_impl(shards, nshards, plan, plan_host, shard, shard_host, m, slot_host, frames_host, n, arena,
                     arena_bytes, arena_rows, arena_nrows, stream);
}
