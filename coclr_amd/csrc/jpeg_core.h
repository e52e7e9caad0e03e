// Baseline JPEG decoding, the per-symbol and per-block arithmetic (include/coclr_hip.h: coclr_jpeg_decode).
// Everything here is `__host__ __device__` and integer only, so the SAME code runs in the gfx950 kernels of
// jpeg.hip and in a g++ build under sanitizers (tools/jpeg_core_check.cpp).  It reproduces libjpeg(-turbo)'s
// default decoder bit for bit: Huffman decoding with zero padding past the data, the "islow" inverse DCT with
// its range table, "fancy" h2v1 / h2v2 chroma upsampling and the 16-bit fixed-point YCbCr -> RGB conversion.
//
// Arithmetic that a corrupt stream can push past 32 bits is done in uint32_t (it wraps, it is never undefined);
// for a stream an encoder wrote, no intermediate leaves the int32 range and the result is libjpeg's.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#define JC_HD __host__ __device__ inline

// ---- per-frame descriptor: int32 words, written by coclr_amd/jpeg.py: pack ---------------------------------------
enum {
  JM_OFF = 0,              // first entropy-coded byte of the frame in the shared byte buffer
  JM_LEN = 1,              // entropy-coded bytes (up to, not including, the marker that ends the scan)
  JM_RI = 2,               // restart interval in MCUs, 0 = none
  JM_NSEG = 3,             // restart segments (1 without restart markers)
  JM_QUANT = 16,           // [3][64] quantiser of component c in natural (row-major) order
  JM_HUFF = JM_QUANT + 192,  // 6 tables of JM_HUFF_WORDS: DC of component 0..2, then AC of component 0..2
  JM_HUFF_WORDS = 96,      //   limit[16], valoff[16], huffval[256] as 64 little-endian words
  JM_SEG = JM_HUFF + 6 * JM_HUFF_WORDS,   // [nseg] first byte of every restart segment, relative to JM_OFF
};
// A code of length l+1 is recognised by peek16 < limit[l] (limit = (last code of that length + 1) << (15 - l),
// non-decreasing in l); its value is huffval[(valoff[l] + (peek16 >> (15 - l))) & 255].

enum { JC_BAD_CODE = 1, JC_BAD_RUN = 2 };   // per-frame status bits

struct jc_geom {
  int H, W, ncomp, hs, vs;     // luma sampling (hs, vs) in {(1,1), (2,1), (2,2)}; chroma is 1x1
  int mcux, mcuy, mcu_blocks;  // MCUs per row / column, blocks per MCU
  int bw[3], bh[3];            // blocks per row / column of every component plane (whole MCUs)
  int boff[3];                 // first block of every component in the frame's coefficient / sample storage
  int nblocks;                 // blocks per frame
  int dw, dh;                  // real size of a chroma plane: ceil(W / hs), ceil(H / vs)
};

JC_HD void jc_geom_init(jc_geom& g, int H, int W, int ncomp, int hs, int vs) {
  g.H = H; g.W = W; g.ncomp = ncomp; g.hs = hs; g.vs = vs;
  g.mcux = (W + 8 * hs - 1) / (8 * hs);
  g.mcuy = (H + 8 * vs - 1) / (8 * vs);
  g.mcu_blocks = ncomp == 1 ? 1 : hs * vs + 2;
  g.nblocks = 0;
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = c < ncomp ? g.mcux * (c == 0 ? hs : 1) : 0;
    g.bh[c] = c < ncomp ? g.mcuy * (c == 0 ? vs : 1) : 0;
    g.boff[c] = g.nblocks;
    g.nblocks += g.bw[c] * g.bh[c];
  }
  g.dw = (W + hs - 1) / hs;
  g.dh = (H + vs - 1) / vs;
}

// ---- bit reader: undoes FF 00 stuffing, stops at a marker or at `end`, yields zero bits from there on ----------------
struct jc_bits {
  const uint8_t* p;
  int pos, end;
  uint64_t buf;      // the next `n` bits, left aligned
  int n;
  int stopped;
};

JC_HD void jc_bits_init(jc_bits& b, const uint8_t* p, int start, int end) {
  b.p = p; b.pos = start; b.end = end; b.buf = 0; b.n = 0; b.stopped = 0;
}

// afterwards at least 57 bits are buffered: one Huffman code (<= 16) and its extra bits (<= 15) need one call
JC_HD void jc_fill(jc_bits& b) {
  while (b.n <= 56) {
    uint32_t c = 0;
    if (!b.stopped && b.pos < b.end) {
      c = b.p[b.pos++];
      if (c == 0xFF) {
        if (b.pos < b.end && b.p[b.pos] == 0) {
          b.pos++;
        } else {
          b.stopped = 1;
          c = 0;
        }
      }
    }
    b.buf |= (uint64_t)c << (56 - b.n);
    b.n += 8;
  }
}

JC_HD uint32_t jc_take(jc_bits& b, int k) {      // 1 <= k <= 16
  const uint32_t v = (uint32_t)(b.buf >> (64 - k));
  b.buf <<= k;
  b.n -= k;
  return v;
}

JC_HD int jc_huff(const int32_t* tab, jc_bits& b, int* status) {
  const uint32_t v = (uint32_t)(b.buf >> 48);
  int l = 0;
  while (l < 16 && v >= (uint32_t)tab[l]) ++l;
  if (l == 16) {                         // no such code: flagged, decoded as 0
    *status |= JC_BAD_CODE;
    jc_take(b, 16);
    return 0;
  }
  const uint32_t idx = ((uint32_t)tab[16 + l] + (v >> (15 - l))) & 255u;
  jc_take(b, l + 1);
  return (int)(((uint32_t)tab[32 + (idx >> 2)] >> ((idx & 3u) * 8u)) & 255u);
}

JC_HD int jc_extend(jc_bits& b, int t) {           // 1 <= t <= 15
  const int v = (int)jc_take(b, t);
  return v >= (1 << (t - 1)) ? v : v - (1 << t) + 1;
}

JC_HD int jc_zigzag(int k) {                       // zigzag position -> natural (row-major) position
  const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

// MCUs m0 .. m1-1 of one frame (one restart segment, or the whole scan): bytes [start, end) of `data` ->
// dequantised coefficients, 64 per block in natural order, at coef[(boff[c] + by * bw[c] + bx) * 64].  `coef` is
// zero-filled by the caller.  One symbol per iteration; the iteration count is bounded by the block count, every
// read stays in [start, end) and every store inside a block of this segment, whatever the bytes and tables hold.
// Returns the status bits.
JC_HD int jc_decode_segment(const uint8_t* data, int start, int end, const int32_t* meta, const jc_geom& g, int m0,
                            int m1, int16_t* coef) {
  jc_bits b;
  jc_bits_init(b, data, start, end);
  int status = 0;
  int dc[3] = {0, 0, 0};
  int mcu = m0, blk = 0, k = 0, comp = 0;
  int16_t* dst = coef;
  const int32_t* q = meta + JM_QUANT;
  const long iters = (long)(m1 - m0) * g.mcu_blocks * 64;
  for (long it = 0; it < iters && mcu < m1; ++it) {
    jc_fill(b);
    if (k == 0) {
      const int luma = g.ncomp == 1 ? 1 : g.hs * g.vs;
      comp = blk < luma ? 0 : blk - luma + 1;
      const int mx = mcu % g.mcux, my = mcu / g.mcux;
      const int bx = comp == 0 ? mx * g.hs + blk % g.hs : mx;
      const int by = comp == 0 ? my * g.vs + blk / g.hs : my;
      dst = coef + ((long)g.boff[comp] + (long)by * g.bw[comp] + bx) * 64;
      q = meta + JM_QUANT + comp * 64;
      const int t = jc_huff(meta + JM_HUFF + comp * JM_HUFF_WORDS, b, &status) & 15;
      const int diff = t ? jc_extend(b, t) : 0;
      dc[comp] = (int16_t)(dc[comp] + diff);
      dst[0] = (int16_t)(dc[comp] * (q[0] & 0xFFFF));
      k = 1;
    } else {
      const int rs = jc_huff(meta + JM_HUFF + (3 + comp) * JM_HUFF_WORDS, b, &status);
      const int r = rs >> 4, s = rs & 15;
      if (s == 0) {
        k = r == 15 ? k + 16 : 64;
      } else {
        k += r;
        if (k > 63) {                     // a run past the block: libjpeg stores it at the last position
          status |= JC_BAD_RUN;
          k = 63;
        }
        const int n = jc_zigzag(k);
        dst[n] = (int16_t)(jc_extend(b, s) * (q[n] & 0xFFFF));
        ++k;
      }
      if (k >= 64) {
        k = 0;
        if (++blk == g.mcu_blocks) {
          blk = 0;
          ++mcu;
        }
      }
    }
  }
  return status;
}

// Restart segment `seg` of the frame described by `m` (width words): its bytes [s0, s1) of the shared buffer of
// data_len bytes and its MCUs [m0, m1).  The descriptor is NOT trusted (a kernel reads the device copy): every value
// is clamped to the buffer, the descriptor's width, `maxseg` and the frame's MCU count.  False: no such segment.
JC_HD int jc_segment_count(const int32_t* m, int width, int maxseg) {      // the clamped count: who decodes the frame
  const int nseg = m[JM_NSEG];
  const int room = width - JM_SEG < maxseg ? width - JM_SEG : maxseg;
  return nseg < 1 ? 1 : nseg > room ? room : nseg;
}

JC_HD bool jc_segment_range(const int32_t* m, int width, int maxseg, int data_len, int seg, const jc_geom& g, int* s0,
                            int* s1, int* m0, int* m1) {
  const int nseg = jc_segment_count(m, width, maxseg);
  if (seg < 0 || seg >= nseg) return false;
  long lo = m[JM_OFF], hi = lo + (long)m[JM_LEN];
  lo = lo < 0 ? 0 : lo > data_len ? data_len : lo;
  hi = hi < lo ? lo : hi > data_len ? data_len : hi;
  long a = lo + m[JM_SEG + seg];
  long b = seg + 1 < nseg ? lo + m[JM_SEG + seg + 1] : hi;
  a = a < lo ? lo : a > hi ? hi : a;
  b = b < a ? a : b > hi ? hi : b;
  const long total = (long)g.mcux * g.mcuy;
  long ri = m[JM_RI];
  if (ri < 1 || ri > total) ri = total;
  long f = seg * ri;
  f = f > total ? total : f;
  long l = f + ri;
  l = l > total ? total : l;
  *s0 = (int)a; *s1 = (int)b; *m0 = (int)f; *m1 = (int)l;
  return true;
}

// ---- inverse DCT: libjpeg's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2) ---------------------------------------------
JC_HD int32_t jc_descale(uint32_t x, int s) { return (int32_t)(x + (1u << (s - 1))) >> s; }

JC_HD void jc_idct_1d(uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3, uint32_t i4, uint32_t i5, uint32_t i6,
                      uint32_t i7, int s, int32_t* o) {
  uint32_t z1 = (i2 + i6) * 4433u;
  const uint32_t t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
  const uint32_t t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a0 = i7, a1 = i5, a2 = i3, a3 = i1;
  z1 = a0 + a3;
  uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  o[0] = jc_descale(t10 + a3, s); o[7] = jc_descale(t10 - a3, s);
  o[1] = jc_descale(t11 + a2, s); o[6] = jc_descale(t11 - a2, s);
  o[2] = jc_descale(t12 + a1, s); o[5] = jc_descale(t12 - a1, s);
  o[3] = jc_descale(t13 + a0, s); o[4] = jc_descale(t13 - a0, s);
}

JC_HD uint8_t jc_range_limit(int32_t x) {          // libjpeg's range table (centre 128), not a clamp
  const int idx = x & 1023;
  return (uint8_t)(idx < 128 ? idx + 128 : idx < 512 ? 255 : idx < 896 ? 0 : idx - 896);
}

// 64 dequantised coefficients in natural order -> 8 x 8 samples at out[y * stride + x]
JC_HD void jc_idct_block(const int16_t* in, uint8_t* out, long stride) {
  int32_t ws[64], o[8];
  for (int c = 0; c < 8; ++c) {
    jc_idct_1d((uint32_t)in[c], (uint32_t)in[8 + c], (uint32_t)in[16 + c], (uint32_t)in[24 + c], (uint32_t)in[32 + c],
               (uint32_t)in[40 + c], (uint32_t)in[48 + c], (uint32_t)in[56 + c], 11, o);
    for (int r = 0; r < 8; ++r) ws[r * 8 + c] = o[r];
  }
  for (int r = 0; r < 8; ++r) {
    const int32_t* w = ws + r * 8;
    jc_idct_1d((uint32_t)w[0], (uint32_t)w[1], (uint32_t)w[2], (uint32_t)w[3], (uint32_t)w[4], (uint32_t)w[5],
               (uint32_t)w[6], (uint32_t)w[7], 18, o);
    for (int c = 0; c < 8; ++c) out[r * stride + c] = jc_range_limit(o[c]);
  }
}

// ---- chroma upsampling (libjpeg-turbo's "fancy" h2v1 / h2v2) and colour conversion ------------------------------------
// Sample of a chroma plane `p` (row stride `pw`, real size dw x dh) at output pixel (x, y), 0 <= x < W, 0 <= y < H.
JC_HD int jc_chroma(const uint8_t* p, long pw, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(long)y * pw + x];
  const int c = x >> 1;
  if (vs == 1) {
    const uint8_t* row = p + (long)y * pw;
    if (x == 0) return row[0];
    if (x == 2 * dw - 1) return row[dw - 1];
    return (x & 1) ? (3 * row[c] + row[c + 1] + 2) >> 2 : (3 * row[c] + row[c - 1] + 1) >> 2;
  }
  const int r = y >> 1;
  int nb = (y & 1) ? r + 1 : r - 1;
  nb = nb < 0 ? 0 : nb > dh - 1 ? dh - 1 : nb;
  const uint8_t* a = p + (long)r * pw;
  const uint8_t* n = p + (long)nb * pw;
  const int cs = 3 * a[c] + n[c];
  if (x == 0) return (4 * cs + 8) >> 4;
  if (x == 2 * dw - 1) return (4 * cs + 7) >> 4;
  if (x & 1) return (3 * cs + 3 * a[c + 1] + n[c + 1] + 7) >> 4;
  return (3 * cs + 3 * a[c - 1] + n[c - 1] + 8) >> 4;
}

JC_HD uint8_t jc_clamp8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

JC_HD void jc_ycc_rgb(int y, int cb, int cr, uint8_t* rgb) {
  cb -= 128;
  cr -= 128;
  rgb[0] = jc_clamp8(y + ((91881 * cr + 32768) >> 16));
  rgb[1] = jc_clamp8(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  rgb[2] = jc_clamp8(y + ((116130 * cb + 32768) >> 16));
}

// One output pixel of a frame from its sample planes (component c at planes + poff[c], row stride pw[c]).
JC_HD void jc_pixel(const uint8_t* planes, const jc_geom& g, int x, int y, uint8_t* rgb) {
  const long pw0 = (long)g.bw[0] * 8;
  const int Y = planes[(long)y * pw0 + x];
  if (g.ncomp == 1) {
    rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;
    return;
  }
  const long pw1 = (long)g.bw[1] * 8;
  const uint8_t* pb = planes + (long)g.boff[1] * 64;
  const uint8_t* pr = planes + (long)g.boff[2] * 64;
  jc_ycc_rgb(Y, jc_chroma(pb, pw1, g.dw, g.dh, g.hs, g.vs, x, y), jc_chroma(pr, pw1, g.dw, g.dh, g.hs, g.vs, x, y),
             rgb);
}

// where block `blk` (0 <= blk < g.nblocks, coefficient order) puts its samples: offset into the frame's planes
JC_HD long jc_block_samples(const jc_geom& g, int blk, long* stride) {
  const int c = blk >= g.boff[2] && g.ncomp == 3 ? 2 : blk >= g.boff[1] && g.ncomp == 3 ? 1 : 0;
  const int i = blk - g.boff[c];
  const int by = i / g.bw[c], bx = i % g.bw[c];
  *stride = (long)g.bw[c] * 8;
  return (long)g.boff[c] * 64 + (long)by * 8 * *stride + bx * 8;
}

// ---- one restart-less segment on many lanes: chunks of raw bytes, decoded from guessed states until they agree ------
// A segment's bytes [s0, s1) are cut into chunks of `chunk_bytes` RAW bytes; a symbol (a Huffman code and its extra
// bits) belongs to the chunk that holds the raw byte of its first bit (the 00 of an FF 00 pair carries no bits).
// Every chunk is scanned from a guessed entry state; each chunk's exit state then becomes the next chunk's entry and
// the chunks whose entry changed are scanned again, until a round changes nothing.  Chunk 0 starts from the true
// state, so after round r chunks 0..r hold the serial decoder's states, and a round without a change has reached
// them everywhere: the result is jc_decode_segment's for ANY bytes, in at most as many rounds as there are chunks.
// jpeg.hip's jpeg_entropy_split_kernel and tools/jpeg_split_check.cpp (host, under sanitizers) drive these functions.
enum { JC_PAST = 0x7fffffff };   // jc_state.pos once the reader has hit `end` or a marker: only zero bits follow

struct jc_state {                // the serial decoder at a symbol boundary, output position aside
  int pos, bit;                  // raw byte that holds the next bit, and the bit within it (0 = the top one)
  int blk, k;                    // block within the MCU (selects the component, so the tables); zigzag index
};

JC_HD jc_state jc_state_make(int pos, int bit, int blk, int k) {
  jc_state s;
  s.pos = pos; s.bit = bit; s.blk = blk; s.k = k;
  return s;
}

JC_HD jc_state jc_state_past() { return jc_state_make(JC_PAST, 0, 0, 0); }

// two words per state, as the kernel keeps them in LDS; states are equal iff their words are
JC_HD int32_t jc_state_word(const jc_state& s) {
  return (int32_t)((uint32_t)s.bit | (uint32_t)s.blk << 3 | (uint32_t)s.k << 8);
}

JC_HD jc_state jc_state_unpack(int32_t pos, int32_t word, const jc_geom& g) {
  const int blk = (word >> 3) & 7;
  return jc_state_make(pos, word & 7, blk < g.mcu_blocks ? blk : 0, (word >> 8) & 63);
}

// jc_bits that also knows which raw byte its next bit came from: per buffered byte one bit "was an FF 00 pair"
// (newest byte = bit 0), and the count of zero bytes pushed behind the end of the real bits (always the newest).
struct jc_cbits : jc_bits {
  uint32_t stuffed;
  int npad;
};

JC_HD void jc_cfill(jc_cbits& b) {                 // the bit stream of jc_fill, byte for byte
  while (b.n <= 56) {
    uint32_t c = 0, s = 0;
    bool real = !b.stopped && b.pos < b.end;
    if (real) {
      c = b.p[b.pos];
      if (c == 0xFF) {
        if (b.pos + 1 < b.end && b.p[b.pos + 1] == 0) {
          s = 1;
        } else {
          b.stopped = 1;
          real = false;
          c = 0;
        }
      }
    }
    if (real) b.pos += 1 + (int)s;
    else if (b.npad < 8) ++b.npad;
    b.stuffed = b.stuffed << 1 | s;
    b.buf |= (uint64_t)c << (56 - b.n);
    b.n += 8;
  }
}

JC_HD void jc_cbits_init(jc_cbits& b, const uint8_t* p, const jc_state& s, int end) {
  jc_bits_init(b, p, s.pos, end);
  b.stuffed = 0;
  b.npad = 0;
  jc_cfill(b);
  if (s.bit) jc_take(b, s.bit);
}

// raw byte of the next bit, JC_PAST when that bit is padding; call after jc_cfill (then 57..64 bits are buffered)
JC_HD int jc_cbits_pos(const jc_cbits& b, int* bit) {
  const int nb = (b.n + 7) >> 3;
  *bit = (8 - (b.n & 7)) & 7;
  if (nb <= b.npad) return JC_PAST;
  const uint32_t pairs = b.stuffed & ((1u << nb) - 1u);
  int cnt = 0;
  for (uint32_t v = pairs; v; v &= v - 1) ++cnt;
  return b.pos - (nb - b.npad) - cnt;
}

// One symbol at zigzag index k of a block of component `comp`, exactly as jc_decode_segment reads it: the next k
// (64: the block is complete), the zigzag index *at the value *val belongs to (0: a DC difference, -1: none).
JC_HD int jc_symbol(const int32_t* meta, jc_cbits& b, int comp, int k, int* at, int* val, int* status) {
  if (k == 0) {
    const int t = jc_huff(meta + JM_HUFF + comp * JM_HUFF_WORDS, b, status) & 15;
    *val = t ? jc_extend(b, t) : 0;
    *at = 0;
    return 1;
  }
  const int rs = jc_huff(meta + JM_HUFF + (3 + comp) * JM_HUFF_WORDS, b, status);
  const int r = rs >> 4, s = rs & 15;
  *at = -1;
  *val = 0;
  if (s == 0) {
    k = r == 15 ? k + 16 : 64;
  } else {
    k += r;
    if (k > 63) {
      *status |= JC_BAD_RUN;
      k = 63;
    }
    *at = k;
    *val = jc_extend(b, s);
    ++k;
  }
  return k >= 64 ? 64 : k;
}

JC_HD long jc_chunk_count(int s0, int s1, int chunk_bytes) {       // at least one: an empty segment still decodes
  const long n = ((long)s1 - s0 + chunk_bytes - 1) / chunk_bytes;
  return n < 1 ? 1 : n;
}

JC_HD int jc_chunk_end(int s0, int s1, int chunk_bytes, long i) {
  const long e = s0 + (i + 1) * chunk_bytes;
  return e > s1 ? s1 : (int)e;
}

// the guess a chunk is first scanned from: bit 0 of its first byte (behind the 00 of an FF 00 pair), block 0, k = 0;
// for chunk 0 this is the true state
JC_HD jc_state jc_chunk_cold(const uint8_t* data, int s0, int s1, int chunk_bytes, long i) {
  long c = s0 + i * chunk_bytes;
  c = c > s1 ? s1 : c;
  if (i > 0 && c < s1 && data[c] == 0 && data[c - 1] == 0xFF) ++c;
  return jc_state_make((int)c, 0, 0, 0);
}

JC_HD int jc_block_comp(const jc_geom& g, int blk) {
  const int luma = g.ncomp == 1 ? 1 : g.hs * g.vs;
  return blk < luma ? 0 : blk - luma + 1;
}

// The symbols that chunk [.., cend) owns, read from entry state `in` (bytes up to `end`, the segment's): the state at
// the first symbol of a later chunk, the blocks completed and, per component, the sum of the DC differences
// (mod 2^16 it is what the serial decoder's int16 predictor gains).  At most 8 * chunk_bytes + 1 symbols.  No status:
// a guessed state meets invalid codes that the real decode never sees.
JC_HD void jc_chunk_scan(const uint8_t* data, int end, int cend, int chunk_bytes, const int32_t* meta, const jc_geom& g,
                         const jc_state& in, jc_state* out, int* blocks, uint32_t* dcsum) {
  *out = in;
  *blocks = 0;
  dcsum[0] = dcsum[1] = dcsum[2] = 0;
  if (in.pos == JC_PAST) return;
  jc_cbits b;
  jc_cbits_init(b, data, in, end);
  int blk = in.blk, k = in.k, ignored = 0;
  const long iters = 8L * chunk_bytes + 1;
  for (long it = 0; it < iters; ++it) {
    jc_cfill(b);
    int bit;
    const int pos = jc_cbits_pos(b, &bit);
    if (pos == JC_PAST) break;
    if (pos >= cend) {
      *out = jc_state_make(pos, bit, blk, k);
      return;
    }
    const int comp = jc_block_comp(g, blk);
    int at, val;
    const int next = jc_symbol(meta, b, comp, k, &at, &val, &ignored);
    if (k == 0) dcsum[comp] += (uint32_t)val;
    k = next;
    if (k == 64) {
      k = 0;
      ++*blocks;
      if (++blk >= g.mcu_blocks) blk = 0;
    }
  }
  *out = jc_state_past();
}

// The same symbols, written: `in` is the chunk's TRUE entry state, `block` the blocks of the segment completed before
// it and dc_in the three DC predictors there.  Coefficients land at jc_decode_segment's addresses with its values
// (coef zero-filled by the caller); the status bits of the owned symbols are returned.  The chunk whose symbols reach
// the end of the real bits carries on over zero bits to the segment's last MCU, as the serial decoder does; a chunk
// entered behind that point writes nothing.  Every store lands inside a block of MCUs [m0, m1).
JC_HD int jc_chunk_write(const uint8_t* data, int end, int cend, int chunk_bytes, const int32_t* meta, const jc_geom& g,
                         const jc_state& in, long block, const int* dc_in, int m0, int m1, int16_t* coef) {
  const long total = (long)(m1 - m0) * g.mcu_blocks;
  if (in.pos == JC_PAST || block < 0 || block >= total) return 0;
  jc_cbits b;
  jc_cbits_init(b, data, in, end);
  int status = 0;
  int dc[3] = {dc_in[0], dc_in[1], dc_in[2]};
  int mcu = m0 + (int)(block / g.mcu_blocks), blk = (int)(block % g.mcu_blocks), k = in.k, comp = 0;
  int16_t* dst = coef;
  const int32_t* q = meta + JM_QUANT;
  bool tail = false, place = true;
  const long iters = 8L * chunk_bytes + 1 + (total - block) * 64;
  for (long it = 0; it < iters && mcu < m1; ++it) {
    jc_cfill(b);
    if (!tail) {
      int bit;
      const int pos = jc_cbits_pos(b, &bit);
      if (pos == JC_PAST) tail = true;
      else if (pos >= cend) break;
    }
    if (place) {
      comp = jc_block_comp(g, blk);
      const int mx = mcu % g.mcux, my = mcu / g.mcux;
      const int bx = comp == 0 ? mx * g.hs + blk % g.hs : mx;
      const int by = comp == 0 ? my * g.vs + blk / g.hs : my;
      dst = coef + ((long)g.boff[comp] + (long)by * g.bw[comp] + bx) * 64;
      q = meta + JM_QUANT + comp * 64;
      place = false;
    }
    int at, val;
    const int next = jc_symbol(meta, b, comp, k, &at, &val, &status);
    if (k == 0) {
      dc[comp] = (int16_t)(dc[comp] + val);
      dst[0] = (int16_t)(dc[comp] * (q[0] & 0xFFFF));
    } else if (at >= 0) {
      const int n = jc_zigzag(at);
      dst[n] = (int16_t)(val * (q[n] & 0xFFFF));
    }
    k = next;
    if (k == 64) {
      k = 0;
      place = true;
      if (++blk >= g.mcu_blocks) {
        blk = 0;
        ++mcu;
      }
    }
  }
  return status;
}

// what the chunks of one window are summed with, in the kernel's scan and on the host alike: block counts saturate at
// the segment's block count (a stream may hold more symbols than the frame has room for), DC sums wrap
JC_HD uint32_t jc_blocks_add(uint32_t a, uint32_t b, uint32_t total) {
  const uint32_t s = (a > total ? total : a) + (b > total ? total : b);
  return s > total ? total : s;
}

// ---- frames of differing geometry in one call (coclr_jpeg_decode_ragged) ---------------------------------------------
// Per frame JR_FIELDS int64 words; `prefix` arrays of F + 1 words hold the lanes (blocks, or row groups of 16 pixels)
// of all frames before each one.  Both are device data to a kernel: nothing read from them is trusted.
enum { JR_H = 0, JR_W, JR_NCOMP, JR_HS, JR_VS, JR_CBLOCK, JR_OBYTE, JR_FIELDS = 8 };

// The frame lane `id` belongs to: the last f in [0, F) with prefix[f] <= id (0 when there is none).  The result is a
// valid frame whatever `prefix` holds; the caller checks id - prefix[f] against the frame's own lane count, which
// also turns away ids past the end.
JC_HD long jc_find_frame(const int64_t* prefix, long F, long id) {
  long lo = 0, hi = F - 1;
  while (lo < hi) {
    const long mid = lo + (hi - lo + 1) / 2;
    if (prefix[mid] <= id) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

JC_HD bool jc_geometry_ok(long H, long W, long ncomp, long hs, long vs, long max_side) {
  if (H < 1 || W < 1 || H > max_side || W > max_side) return false;
  if (ncomp == 1) return hs == 1 && vs == 1;
  return ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}

// Frame f of the table `tab`: its geometry, its first block in the coefficient / sample storage of coef_blocks blocks
// and its first byte in the output of out_bytes bytes.  False (the frame is skipped) unless the geometry is one the
// kernels take and both ranges lie inside their buffers, so every address derived from a frame that passes is inside.
JC_HD bool jc_ragged_frame(const int64_t* tab, long f, long coef_blocks, long out_bytes, long max_side, jc_geom& g,
                           long* cblock, long* obyte) {
  const int64_t* t = tab + f * JR_FIELDS;
  if (!jc_geometry_ok(t[JR_H], t[JR_W], t[JR_NCOMP], t[JR_HS], t[JR_VS], max_side)) return false;
  jc_geom_init(g, (int)t[JR_H], (int)t[JR_W], (int)t[JR_NCOMP], (int)t[JR_HS], (int)t[JR_VS]);
  const long cb = t[JR_CBLOCK], ob = t[JR_OBYTE];
  if (cb < 0 || cb > coef_blocks - g.nblocks) return false;
  if (ob < 0 || ob > out_bytes - (long)g.H * g.W * 3) return false;
  *cblock = cb;
  *obyte = ob;
  return true;
}

JC_HD long jc_row_groups(const jc_geom& g) { return (long)g.H * ((g.W + 15) / 16); }   // colour lanes of a frame

// ---- a device-resident store of frames, decoded by index (coclr_jpeg_store_index, coclr_jpeg_decode_store) ----------
// Per frame JS_FIELDS int64 words.  The JM_QUANT .. JM_SEG words of a descriptor are kept once per distinct table set:
// set i lies at tables[JS_TABLE_PAD + i * JS_TABLE_WORDS], so tables + i * JS_TABLE_WORDS serves as `meta` for every
// function above that reads only JM_QUANT / JM_HUFF.  Segment offsets of frames with restart markers lie in one flat
// int32 array.  A restart-less frame (JS_NSEG == 1) has one row of JS_ROW_WORDS words per chunk of chunk_bytes raw
// bytes: the serial decoder's state at the chunk's first symbol, which jc_chunk_write decodes the chunk from.
// All of it is device data to a kernel: jc_store_frame_get clamps whatever a record holds to the buffers.
enum {
  JS_BASE = 0,             // first entropy-coded byte of the frame in the store's bytes, 64 bits
  JS_LEN,                  // entropy-coded bytes, < 2^31
  JS_RI,                   // restart interval in MCUs, 0 = none
  JS_NSEG,                 // restart segments (1: decoded by chunk from its rows)
  JS_TSET,                 // table set
  JS_SEG,                  // first of its JS_NSEG words in the segment array (JS_NSEG > 1)
  JS_ROW,                  // first of its chunk rows (JS_NSEG == 1)
  JS_GEOM,                 // jc_geom_pack
  JS_FIELDS = 8,
  JS_TABLE_WORDS = JM_SEG - JM_QUANT,
  JS_TABLE_PAD = JM_QUANT,
  JS_ROW_WORDS = 4,
};

JC_HD int64_t jc_geom_pack(long H, long W, long ncomp, long hs, long vs) {
  return (int64_t)(H | W << 16 | ncomp << 32 | hs << 36 | vs << 40);
}

struct jc_store_frame {
  const uint8_t* bytes;    // the frame's first byte: positions below are relative to it
  int len, nseg;
  long ri, seg, row;
  const int32_t* meta;     // displaced: meta[JM_QUANT ..] and meta[JM_HUFF ..] are the frame's table set
  long H, W, ncomp, hs, vs;    // as recorded; not checked (jc_geometry_ok)
};

JC_HD void jc_store_frame_get(const int64_t* rec, const uint8_t* data, int64_t data_bytes, const int32_t* tables,
                              long table_sets, jc_store_frame& o) {
  int64_t base = rec[JS_BASE], len = rec[JS_LEN], ts = rec[JS_TSET], nseg = rec[JS_NSEG];
  base = base < 0 ? 0 : base > data_bytes ? data_bytes : base;
  len = len < 0 ? 0 : len > data_bytes - base ? data_bytes - base : len;
  len = len > 0x7fffffff ? 0x7fffffff : len;
  ts = ts < 0 || ts >= table_sets ? 0 : ts;
  o.bytes = data + base;
  o.len = (int)len;
  o.nseg = nseg < 1 ? 1 : nseg > 0x7fffffff ? 0x7fffffff : (int)nseg;
  o.ri = rec[JS_RI];
  o.seg = rec[JS_SEG];
  o.row = rec[JS_ROW];
  o.meta = tables + ts * JS_TABLE_WORDS;
  const int64_t p = rec[JS_GEOM];
  o.H = p & 0xFFFF; o.W = p >> 16 & 0xFFFF; o.ncomp = p >> 32 & 15; o.hs = p >> 36 & 15; o.vs = p >> 40 & 15;
}

// jc_segment_range for a frame of the store: segment `seg` of its f.nseg, offsets from the flat array `segs` of nsegs
// words; bytes [s0, s1) relative to f.bytes, MCUs [m0, m1).  False: no such segment, or its words leave the array.
JC_HD bool jc_store_segment(const jc_store_frame& f, const int32_t* segs, long nsegs, long seg, const jc_geom& g, int* s0,
                            int* s1, int* m0, int* m1) {
  if (seg < 0 || seg >= f.nseg || f.seg < 0 || f.seg > nsegs - f.nseg) return false;
  const long hi = f.len;
  long a = segs[f.seg + seg];
  long b = seg + 1 < f.nseg ? segs[f.seg + seg + 1] : hi;
  a = a < 0 ? 0 : a > hi ? hi : a;
  b = b < a ? a : b > hi ? hi : b;
  const long total = (long)g.mcux * g.mcuy;
  long ri = f.ri;
  if (ri < 1 || ri > total) ri = total;
  long first = seg > total ? total : seg * ri;
  first = first > total ? total : first;
  long last = first + ri;
  last = last > total ? total : last;
  *s0 = (int)a; *s1 = (int)b; *m0 = (int)first; *m1 = (int)last;
  return true;
}

// A chunk's row: word 0 = jc_state_word (14 bits) | (pos - first byte of the chunk) << 14 (17 bits) | past << 31,
// word 1 = blocks of the frame completed before the chunk, word 2 = DC predictor 0 | predictor 1 << 16, word 3 =
// predictor 2; a past state is word 0 = 1 << 31 and zeros.  A true entry lies within a symbol's length (8 raw bytes at most, FF 00 pairs included) of its chunk.
JC_HD void jc_row_pack(uint32_t* row, const jc_state& s, long chunk_start, uint32_t blocks, const uint32_t* dc) {
  if (s.pos == JC_PAST) {                                  // one form: such a chunk writes nothing
    row[0] = 1u << 31;
    row[1] = row[2] = row[3] = 0;
    return;
  } else {
    long rel = (long)s.pos - chunk_start;
    rel = rel < 0 ? 0 : rel > 0x1FFFF ? 0x1FFFF : rel;
    row[0] = ((uint32_t)jc_state_word(s) & 0x3FFFu) | (uint32_t)rel << 14;
  }
  row[1] = blocks;
  row[2] = (dc[0] & 0xFFFFu) | dc[1] << 16;
  row[3] = dc[2] & 0xFFFFu;
}

// The state a row holds for the chunk that starts at chunk_start of a frame of `len` bytes.  Whatever the words are,
// the position lies in [chunk_start, len] and block and k are ones jc_chunk_write takes.
JC_HD jc_state jc_row_unpack(const uint32_t* row, long chunk_start, int len, const jc_geom& g, long* blocks, int* dc) {
  *blocks = (long)row[1];
  dc[0] = (int16_t)(row[2] & 0xFFFFu);
  dc[1] = (int16_t)(row[2] >> 16);
  dc[2] = (int16_t)(row[3] & 0xFFFFu);
  if (row[0] >> 31) return jc_state_past();
  long pos = chunk_start + (long)(row[0] >> 14 & 0x1FFFFu);
  pos = pos > len ? len : pos;
  return jc_state_unpack((int32_t)pos, (int32_t)(row[0] & 0x3FFFu), g);
}

JC_HD long jc_chunk_start(int len, int chunk_bytes, long i) {
  const long c = i * chunk_bytes;
  return c > len ? len : c;
}

// the entropy lanes of a store frame: its chunks, or its restart segments
JC_HD long jc_store_lanes(int len, int nseg, int chunk_bytes) {
  return nseg == 1 ? jc_chunk_count(0, len, chunk_bytes) : nseg;
}

// ---- a pixel box of a store frame, decoded alone (coclr_jpeg_decode_store_window) ------------------------------------
// Per frame JW_FIELDS int64 words: the box x0, y0, w, h inside the frame.  Coefficients and sample planes keep the
// full-frame layout of jc_geom, so every function above addresses and computes as it does for a whole frame; fewer
// lanes run.  What must be decoded is the MCU rectangle [mx0, mx1) x [my0, my1) that holds every sample jc_pixel
// reads for the box's pixels: the luma samples of the box, and on an axis subsampled by 2 the chroma columns or rows
// (p >> 1) - 1 .. (p >> 1) + 1 that jc_chroma touches, clamped to the plane's real size dw / dh as jc_chroma clamps.
enum { JW_X0 = 0, JW_Y0, JW_W, JW_H, JW_FIELDS = 4 };

struct jc_window {
  int x0, y0, w, h;            // the box, inside the frame
  int mx0, my0, mx1, my1;      // its MCU rectangle
};

// False: the box is empty or leaves the frame (nothing of `o` is then to be used).
JC_HD bool jc_window_init(const jc_geom& g, long x0, long y0, long w, long h, jc_window& o) {
  if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || x0 > g.W - w || y0 > g.H - h) return false;
  o.x0 = (int)x0; o.y0 = (int)y0; o.w = (int)w; o.h = (int)h;
  const int xl = (int)(x0 + w - 1), yl = (int)(y0 + h - 1);
  o.mx0 = o.x0 / (8 * g.hs);
  o.mx1 = xl / (8 * g.hs);
  o.my0 = o.y0 / (8 * g.vs);
  o.my1 = yl / (8 * g.vs);
  if (g.ncomp == 3 && g.hs == 2) {
    int lo = (o.x0 >> 1) - 1, hi = (xl >> 1) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > g.dw - 1 ? g.dw - 1 : hi;
    o.mx0 = lo / 8 < o.mx0 ? lo / 8 : o.mx0;
    o.mx1 = hi / 8 > o.mx1 ? hi / 8 : o.mx1;
  }
  if (g.ncomp == 3 && g.vs == 2) {
    int lo = (o.y0 >> 1) - 1, hi = (yl >> 1) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > g.dh - 1 ? g.dh - 1 : hi;
    o.my0 = lo / 8 < o.my0 ? lo / 8 : o.my0;
    o.my1 = hi / 8 > o.my1 ? hi / 8 : o.my1;
  }
  ++o.mx1;
  ++o.my1;
  return true;
}

JC_HD long jc_window_blocks(const jc_geom& g, const jc_window& o) {         // inverse-DCT lanes of a window
  return (long)(o.mx1 - o.mx0) * (o.my1 - o.my0) * g.mcu_blocks;
}

JC_HD long jc_window_row_groups(const jc_window& o) { return (long)o.h * ((o.w + 15) / 16); }   // colour lanes

JC_HD long jc_window_first(const jc_geom& g, const jc_window& o) { return (long)o.my0 * g.mcux + o.mx0; }
JC_HD long jc_window_last(const jc_geom& g, const jc_window& o) { return (long)(o.my1 - 1) * g.mcux + o.mx1; }

// Block `local` (0 <= local < jc_window_blocks) of the window -> its index in the FULL frame's coefficient order: the
// window's luma blocks row by row, then its Cb blocks, then its Cr blocks.
JC_HD int jc_window_block(const jc_geom& g, const jc_window& o, long local) {
  const long mcus = (long)(o.mx1 - o.mx0) * (o.my1 - o.my0);
  const long luma = g.ncomp == 1 ? mcus : mcus * g.hs * g.vs;
  const int c = local < luma ? 0 : local < luma + mcus ? 1 : 2;
  const long i = c == 0 ? local : local - luma - (c - 1) * mcus;
  const int sx = c == 0 ? g.hs : 1, sy = c == 0 ? g.vs : 1;
  const int wb = (o.mx1 - o.mx0) * sx;
  const int by = o.my0 * sy + (int)(i / wb), bx = o.mx0 * sx + (int)(i % wb);
  return g.boff[c] + by * g.bw[c] + bx;
}

// An entropy lane that touches blocks b0 .. b1 of the frame (a chunk: the blocks completed before it through those
// completed before the next chunk -- the block in progress at the boundary has symbols in both) decodes nothing the
// window needs when the range lies wholly before the window's first MCU or starts at or after the end of its last.
JC_HD bool jc_window_skips_blocks(const jc_geom& g, const jc_window& o, long b0, long b1) {
  return b1 < jc_window_first(g, o) * g.mcu_blocks || b0 >= jc_window_last(g, o) * g.mcu_blocks;
}

JC_HD bool jc_window_skips_mcus(const jc_geom& g, const jc_window& o, long m0, long m1) {     // a restart segment
  return m1 <= jc_window_first(g, o) || m0 >= jc_window_last(g, o);
}

// jc_ragged_frame for a window: frame f's geometry and first block as there, its box from `win`, and its first output
// byte checked for the 3 * w * h bytes the box takes.  False (the frame is skipped) unless all of it holds.
JC_HD bool jc_window_frame(const int64_t* tab, const int64_t* win, long f, long coef_blocks, long out_bytes,
                           long max_side, jc_geom& g, jc_window& o, long* cblock, long* obyte) {
  const int64_t* t = tab + f * JR_FIELDS;
  const int64_t* b = win + f * JW_FIELDS;
  if (!jc_geometry_ok(t[JR_H], t[JR_W], t[JR_NCOMP], t[JR_HS], t[JR_VS], max_side)) return false;
  jc_geom_init(g, (int)t[JR_H], (int)t[JR_W], (int)t[JR_NCOMP], (int)t[JR_HS], (int)t[JR_VS]);
  if (!jc_window_init(g, b[JW_X0], b[JW_Y0], b[JW_W], b[JW_H], o)) return false;
  const long cb = t[JR_CBLOCK], ob = t[JR_OBYTE];
  if (cb < 0 || cb > coef_blocks - g.nblocks) return false;
  if (ob < 0 || ob > out_bytes - (long)o.w * o.h * 3) return false;
  *cblock = cb;
  *obyte = ob;
  return true;
}

// ---- a selection of store frames copied to a device arena (coclr_jpeg_store_gather) ---------------------------------
// The store's bytes and rows may lie in pinned host memory; a call's distinct frames are copied to a device arena, 16
// bytes per lane, and decoded there through records rebased to the arena.  Frame j's first arena byte is congruent to
// its first store byte mod 16, so the copy is one of whole aligned 16-byte words: the frame's HULL, words
// [base >> 4, (base + len + 15) >> 4).  Every word of a hull holds a byte of the frame, so a hull never leaves the
// 16-byte words its buffer's bytes touch.  An empty frame has no hull.  Hulls follow each other in the arena without a
// gap and never share a word; what a hull holds outside its frame is copied and never read.  Rows are 16 bytes each.
// Per distinct frame JG_FIELDS int64 words; a lane finds its frame by binary search over the JG_LANE column.  The plan
// is device data to the kernel: every word address derived from it is held against the buffers' sizes, which are
// kernel arguments.
enum {
  JG_FRAME = 0,            // the store frame
  JG_SRC,                  // its first byte in the store (JS_BASE)
  JG_LEN,                  // its bytes (JS_LEN)
  JG_DST,                  // its first byte in the arena, congruent to JG_SRC mod 16
  JG_SRCROW,               // its first row in the store (JS_ROW)
  JG_NROWS,                // its rows: jc_chunk_count for a frame of one restart segment, else 0
  JG_DSTROW,               // its first row in the arena
  JG_LANE,                 // lanes (hull words, then rows) of all frames before it
  JG_FIELDS = 8,
};

struct jc_span {
  int64_t src, dst, words;     // first 16-byte word in the store and in the arena, and how many
};

// The hull of `len` bytes at store byte `src`, to be copied to arena byte `dst`.  False: a negative or overflowing
// range, a frame of 2^31 bytes or more, or a `dst` that is not congruent to `src` mod 16.
JC_HD bool jc_gather_span(int64_t src, int64_t len, int64_t dst, jc_span& o) {
  const int64_t top = (int64_t)1 << 62;
  if (src < 0 || dst < 0 || len < 0 || len > 0x7fffffff || src > top || dst > top || ((src ^ dst) & 15)) return false;
  o.src = src >> 4;
  o.dst = dst >> 4;
  o.words = len == 0 ? 0 : ((src + len + 15) >> 4) - (src >> 4);
  return true;
}

// where a frame whose store byte is `src` goes when the hulls before it end at arena byte `end` (a multiple of 16),
// and where its own hull ends
JC_HD int64_t jc_gather_place(int64_t end, int64_t src) { return end + (src & 15); }
JC_HD int64_t jc_gather_end(const jc_span& s) { return (s.dst + s.words) << 4; }

// The rows a store frame brings: false when the record's bytes leave the store's `data_bytes` or its rows the store's
// `nrows` (the refusal of coclr_jpeg_store_gather; frames with restart markers bring none).
JC_HD bool jc_gather_frame_ok(const int64_t* rec, int64_t data_bytes, int64_t nrows, int chunk_bytes, int64_t* brings) {
  const int64_t base = rec[JS_BASE], len = rec[JS_LEN], nseg = rec[JS_NSEG], row = rec[JS_ROW];
  if (base < 0 || len < 0 || len > 0x7fffffff || data_bytes < len || base > data_bytes - len || nseg < 1) return false;
  *brings = nseg == 1 ? jc_chunk_count(0, (int)len, chunk_bytes) : 0;
  return *brings == 0 || (row >= 0 && nrows >= *brings && row <= nrows - *brings);
}

// the record of a frame in the arena: its own, with the first byte and the first row replaced
JC_HD void jc_gather_rebase(const int64_t* rec, int64_t dst, int64_t dstrow, int64_t* out) {
  for (int i = 0; i < JS_FIELDS; ++i) out[i] = rec[i];
  out[JS_BASE] = dst;
  out[JS_ROW] = dstrow;
}

// jc_find_frame over the JG_LANE column of a plan of m frames
JC_HD long jc_gather_find(const int64_t* plan, long m, int64_t id) {
  long lo = 0, hi = m - 1;
  while (lo < hi) {
    const long mid = lo + (hi - lo + 1) / 2;
    if (plan[mid * JG_FIELDS + JG_LANE] <= id) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// A sharded gather is the same gather with a SOURCE per plan row: the shards of a store lie in different buffers (the
// memory of this rank, or a peer's mapped through hipIpc), at most JG_MAX_SHARDS of them, one per GPU of a node.  The
// int64 column shard[m] names row j's source; JG_FRAME, JG_SRC and JG_SRCROW then count inside THAT shard.  The rules
// of placement are unchanged -- the congruence is to the frame's first shard byte -- and the rows of a plan are ordered
// by (shard, frame).
enum { JG_MAX_SHARDS = 8 };

struct jc_gather_size {
  int64_t words, nrows;        // one source: the 16-byte words its bytes touch, and its rows
};

// Lane `id` of a gather over `nshards` sources: which 16-byte word it copies, and from which source.  `Src` is any
// struct with the members of jc_gather_size (the kernel's table entry carries the two pointers as well); `shard`
// null: every row reads source 0.  `rows` says whether the word is a row (then src / dst count rows) or a word of the
// bytes.  False: the lane has nothing to copy, its row names a source outside [0, nshards), or its words leave THAT
// source or the arena (sizes in words).  Plan and shard column are device data: nothing read from them is trusted.
template <class Src>
JC_HD bool jc_gather_lane_from(const int64_t* plan, const int64_t* shard, long m, int64_t id, const Src* srcs,
                               int64_t nshards, int64_t dst_words, int64_t dst_rows, int64_t* which, bool* rows,
                               int64_t* src, int64_t* dst) {
  const long j = jc_gather_find(plan, m, id);
  const int64_t* p = plan + j * JG_FIELDS;
  const int64_t w = shard ? shard[j] : 0;
  if (w < 0 || w >= nshards) return false;
  *which = w;
  int64_t local = id - p[JG_LANE];
  jc_span s;
  if (local < 0 || !jc_gather_span(p[JG_SRC], p[JG_LEN], p[JG_DST], s)) return false;
  if (local < s.words) {
    *rows = false;
    *src = s.src + local;
    *dst = s.dst + local;
    return *src < srcs[w].words && *dst < dst_words;
  }
  local -= s.words;
  const int64_t top = (int64_t)1 << 62;
  if (local >= p[JG_NROWS] || p[JG_SRCROW] < 0 || p[JG_DSTROW] < 0 || p[JG_SRCROW] > top || p[JG_DSTROW] > top)
    return false;
  *rows = true;
  *src = p[JG_SRCROW] + local;
  *dst = p[JG_DSTROW] + local;
  return *src < srcs[w].nrows && *dst < dst_rows;
}

// the gather of ONE source (coclr_jpeg_store_gather): the one-shard case of the above
JC_HD bool jc_gather_lane(const int64_t* plan, long m, int64_t id, int64_t src_words, int64_t src_rows,
                          int64_t dst_words, int64_t dst_rows, bool* rows, int64_t* src, int64_t* dst) {
  const jc_gather_size one = {src_words, src_rows};
  int64_t which;
  return jc_gather_lane_from(plan, (const int64_t*)nullptr, m, id, &one, 1, dst_words, dst_rows, &which, rows, src,
                             dst);
}

// Row j of a sharded plan against the row before it: its source exists and the rows are ordered by (shard, frame),
// strictly -- a plan holds DISTINCT frames (the refusal of coclr_jpeg_store_gather_shards).
JC_HD bool jc_gather_order_ok(const int64_t* plan, const int64_t* shard, long j, int64_t nshards) {
  const int64_t w = shard[j], f = plan[j * JG_FIELDS + JG_FRAME];
  if (w < 0 || w >= nshards || f < 0) return false;
  if (j == 0) return true;
  const int64_t pw = shard[j - 1], pf = plan[(j - 1) * JG_FIELDS + JG_FRAME];
  return pw < w || (pw == w && pf < f);
}
