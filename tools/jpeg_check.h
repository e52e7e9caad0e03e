// What the host check programs tools/jpeg_{core,split,ragged,store,window}_check.cpp share: the cases file and its
// reader, the seeded damage generator, and the two host restatements every check of the chunked decoders leans on --
// relax_windows, the order in which jpeg_entropy_split_kernel and jpeg_store_index_kernel find the chunks' true states,
// and serial_rows, the same states from one serial walk.  Each program is one translation unit that includes this file.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../coclr_amd/csrc/jpeg_core.h"

constexpr int LANES = 1024;            // the kernels' largest workgroup: chunks per window

// The cases file is little-endian int32 words and bytes, written by tests/_jpeg_cases.py: write_core_check_cases from
// coclr_amd.jpeg.pack:
//   magic 0x4A504731, case count, then per case
//   H, W, components, hs, vs, descriptor width, byte count, corrupt (0 / 1),
//   descriptor[width] int32, the entropy-coded bytes, the expected H * W * 3 RGB bytes.
struct Case {
  int H, W, ncomp, hs, vs, width, len, corrupt;
  std::vector<int32_t> meta;           // JM_OFF is 0: a case's bytes stand alone
  std::vector<uint8_t> data;
  std::vector<uint8_t> rgb;            // the expected bytes; empty unless read_cases was asked to keep them
  std::vector<int32_t> boxes;          // [n][4] pixel boxes; jpeg_window_check.cpp fills them from its second file
};

inline bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// false: the file cannot be read, or a case in it is not one the kernels' entry points would take
inline bool read_cases(const char* path, bool keep_rgb, std::vector<Case>& cases) {
  FILE* f = fopen(path, "rb");
  int32_t head[2];
  if (!f || !read_exact(f, head, sizeof head) || head[0] != 0x4A504731 || head[1] < 1) return false;
  cases.resize(head[1]);
  for (Case& c : cases) {
    int32_t h[8];
    if (!read_exact(f, h, sizeof h)) return false;
    c.H = h[0]; c.W = h[1]; c.ncomp = h[2]; c.hs = h[3]; c.vs = h[4]; c.width = h[5]; c.len = h[6]; c.corrupt = h[7];
    if (!jc_geometry_ok(c.H, c.W, c.ncomp, c.hs, c.vs, 8192) || c.width <= JM_SEG || c.width > (1 << 20) || c.len < 0)
      return false;
    c.meta.resize(c.width);
    c.data.resize(c.len);
    const size_t pixels = (size_t)c.H * c.W * 3;
    if (!read_exact(f, c.meta.data(), (size_t)c.width * 4) || !read_exact(f, c.data.data(), c.len)) return false;
    if (keep_rgb) {
      c.rgb.resize(pixels);
      if (!read_exact(f, c.rgb.data(), pixels)) return false;
    } else if (fseek(f, (long)pixels, SEEK_CUR) != 0) {
      return false;
    }
    if (c.meta[JM_NSEG] < 1 || c.meta[JM_NSEG] > c.width - JM_SEG) return false;
    c.meta[JM_OFF] = 0;
  }
  fclose(f);
  return true;
}

// the seeded generator of every damaged stream
inline uint32_t lcg(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return s >> 8;
}

inline bool same(const jc_state& a, const jc_state& b) { return a.pos == b.pos && jc_state_word(a) == jc_state_word(b); }

// One segment [s0, s1) of `total` blocks in chunks, in the kernels' order (jpeg.hip: split_windows): windows of LANES
// chunks, each starting from the converged exit of the one before and none once that exit is past the real bits; in a
// window cold scans, then rounds in which ALL chunks read the previous round's exits and those whose entry changed scan
// again, until a round changes nothing; then a prefix of block counts (saturating at total) and DC sums, in front of
// which lies the carry of the windows before.  Per chunk, in order,
//   emit(chunk, its true entry, its exit, blocks of the segment completed before it, the three DC sums there).
// Returns the first chunk no window reached and, per window, how many rounds changed an entry.
struct Relaxed {
  long reached;
  std::vector<long> rounds;
};

template <class Emit>
Relaxed relax_windows(const uint8_t* data, int s0, int s1, const int32_t* meta, const jc_geom& g, uint32_t total,
                      int chunk_bytes, Emit emit) {
  const long nchunks = jc_chunk_count(s0, s1, chunk_bytes);
  Relaxed res = {0, {}};
  jc_state first = jc_state_make(s0, 0, 0, 0);
  uint32_t block = 0, dc[3] = {0, 0, 0};
  std::vector<jc_state> in(LANES), out(LANES), prev(LANES);
  std::vector<int> blocks(LANES);
  std::vector<uint32_t> dcs((size_t)LANES * 3);
  long w0 = 0;
  for (; w0 < nchunks; w0 += LANES) {
    if (first.pos == JC_PAST) break;
    const int n = (int)(nchunks - w0 < LANES ? nchunks - w0 : LANES);
    auto scan = [&](int t) {
      jc_chunk_scan(data, s1, jc_chunk_end(s0, s1, chunk_bytes, w0 + t), chunk_bytes, meta, g, in[t], &out[t],
                    &blocks[t], &dcs[(size_t)t * 3]);
    };
    for (int t = 0; t < n; ++t) {
      in[t] = t == 0 ? first : jc_chunk_cold(data, s0, s1, chunk_bytes, w0 + t);
      scan(t);
    }
    long rounds = 0;
    for (int r = 0; r < LANES; ++r) {
      prev = out;                                  // every chunk reads the previous round's exits
      bool any = false;
      for (int t = 1; t < n; ++t)
        if (!same(prev[t - 1], in[t])) {
          in[t] = prev[t - 1];
          scan(t);
          any = true;
        }
      if (!any) break;
      ++rounds;
    }
    res.rounds.push_back(rounds);
    for (int t = 0; t < n; ++t) {
      emit(w0 + t, in[t], out[t], block, dc);
      block = jc_blocks_add(block, (uint32_t)blocks[t], total);
      for (int c = 0; c < 3; ++c) dc[c] += dcs[(size_t)t * 3 + c];
    }
    first = out[n - 1];
  }
  res.reached = w0;
  return res;
}

// The rows of a frame of one restart segment (jc_row_pack) from ONE serial walk over its bytes: the decoder's state
// whenever a symbol is the first to start in a later chunk.
inline void serial_rows(const uint8_t* data, int len, const int32_t* meta, const jc_geom& g, int cb,
                        std::vector<uint32_t>& rows) {
  const long nchunks = jc_chunk_count(0, len, cb);
  const uint64_t total = (uint64_t)((long)g.mcux * g.mcuy * g.mcu_blocks);
  rows.assign((size_t)nchunks * JS_ROW_WORDS, 0xDEADBEEFu);
  uint32_t dc[3] = {0, 0, 0};
  uint64_t blocks = 0;
  jc_row_pack(&rows[0], jc_state_make(0, 0, 0, 0), 0, 0, dc);      // chunk 0 starts where the frame does
  long next = 1;
  jc_cbits b;
  jc_cbits_init(b, data, jc_state_make(0, 0, 0, 0), len);
  int blk = 0, k = 0, ignored = 0;
  for (;;) {
    jc_cfill(b);
    int bit;
    const int pos = jc_cbits_pos(b, &bit);
    if (pos == JC_PAST) break;
    for (; next < nchunks && pos >= jc_chunk_start(len, cb, next); ++next)
      jc_row_pack(&rows[(size_t)next * JS_ROW_WORDS], jc_state_make(pos, bit, blk, k), jc_chunk_start(len, cb, next),
                  (uint32_t)(blocks > total ? total : blocks), dc);
    const int comp = jc_block_comp(g, blk);
    int at, val;
    const int nk = jc_symbol(meta, b, comp, k, &at, &val, &ignored);
    if (k == 0) dc[comp] += (uint32_t)val;
    k = nk;
    if (k == 64) {
      k = 0;
      ++blocks;
      if (++blk >= g.mcu_blocks) blk = 0;
    }
  }
  for (; next < nchunks; ++next) jc_row_pack(&rows[(size_t)next * JS_ROW_WORDS], jc_state_past(), 0, 0, dc);
}
