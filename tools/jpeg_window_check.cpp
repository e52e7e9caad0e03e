// Host check of the window arithmetic of coclr_amd/csrc/jpeg_core.h (jc_window_init, jc_window_block,
// jc_window_skips_blocks / jc_window_skips_mcus), the code that the window forms of jpeg_entropy_store_kernel,
// jpeg_idct_kernel and jpeg_colour_kernel run (tests/test_jpeg_window_cpu.py builds this with
// g++ -fsanitize=address,undefined -fno-sanitize-recover=all and runs it on tests/golden/jpeg_frames.pt):
//
//   jpeg_window_check <cases file> <boxes file>
//
// The cases file is the one tools/jpeg_core_check.cpp reads (tests/_jpeg_cases.py: write_core_check_cases); the boxes
// file lists per case its pixel boxes (tests/_jpeg_window_cases.py: write_boxes).  For every case, at chunk sizes 8 and
// 64, and every box:
//   rows     one serial walk over the bytes notes the decoder's state at the first symbol of every chunk (serial_rows of
//            tools/jpeg_check.h, once per case and chunk size; the store's rows, tools/jpeg_store_check.cpp ties the
//            kernel's order to this walk);
//   entropy  what a lane of the window kernel does, per chunk, last chunk first: its own row and the next row's block
//            count, the skip predicate, jc_chunk_write with m1 = the window's last MCU -- or per restart segment the
//            segment predicate and jc_decode_segment -- into zero-filled coefficients in an exact heap block;
//   compare  the blocks of the window's MCU rectangle equal the full decode's, every block of an MCU at or after the
//            window's last is zero (restart-less frames), and so is every block of MCUs whose lanes were all skipped;
//   idct     jc_window_block / jc_block_samples / jc_idct_block for every block of the rectangle, into sample planes
//            filled with 0x5a everywhere else;
//   pixels   jc_pixel at the box's pixels equals the crop of the golden RGB frame (PIL's bytes);
//   reads    every sample jc_pixel reads for a pixel of the box -- the luma sample, and the chroma columns and rows
//            jc_chroma addresses, listed here from its definition -- lies in a block of the MCU rectangle.
// Exit 0 = all held.
#include "jpeg_check.h"

namespace {

struct Tally {
  long windows = 0, lanes = 0, skipped = 0, blocks = 0, pixels = 0, reads = 0, failed = 0;
};

// the MCU a block of the frame (coefficient order) belongs to
long block_mcu(const jc_geom& g, int blk) {
  const int c = blk >= g.boff[2] && g.ncomp == 3 ? 2 : blk >= g.boff[1] && g.ncomp == 3 ? 1 : 0;
  const int i = blk - g.boff[c], by = i / g.bw[c], bx = i % g.bw[c];
  const int mx = c == 0 ? bx / g.hs : bx, my = c == 0 ? by / g.vs : by;
  return (long)my * g.mcux + mx;
}

bool mcu_in_rect(const jc_geom& g, const jc_window& w, long mcu) {
  const int mx = (int)(mcu % g.mcux), my = (int)(mcu / g.mcux);
  return mx >= w.mx0 && mx < w.mx1 && my >= w.my0 && my < w.my1;
}

// sample (sx, sy) of component c lies in a block of the rectangle
bool sample_in_rect(const jc_geom& g, const jc_window& w, int c, int sx, int sy) {
  if (sx < 0 || sy < 0 || sx >= g.bw[c] * 8 || sy >= g.bh[c] * 8) return false;
  const int mx = c == 0 ? sx / (8 * g.hs) : sx / 8, my = c == 0 ? sy / (8 * g.vs) : sy / 8;
  return mx >= w.mx0 && mx < w.mx1 && my >= w.my0 && my < w.my1;
}

// every sample jc_pixel reads for pixel (x, y), from jc_chroma's definition
bool reads_inside(const jc_geom& g, const jc_window& w, int x, int y, long* reads) {
  bool ok = sample_in_rect(g, w, 0, x, y);
  ++*reads;
  if (g.ncomp == 1) return ok;
  int cols[2], ncols = 0, rows[2], nrows = 0;
  if (g.hs == 1) {
    cols[ncols++] = x;
  } else {
    const int c = x >> 1;
    cols[ncols++] = c;
    if (x != 0 && x != 2 * g.dw - 1) cols[ncols++] = (x & 1) ? c + 1 : c - 1;
  }
  if (g.vs == 1) {
    rows[nrows++] = y;
  } else {
    const int r = y >> 1;
    int nb = (y & 1) ? r + 1 : r - 1;
    nb = nb < 0 ? 0 : nb > g.dh - 1 ? g.dh - 1 : nb;
    rows[nrows++] = r;
    rows[nrows++] = nb;
  }
  for (int c = 1; c < 3; ++c)
    for (int i = 0; i < ncols; ++i)
      for (int j = 0; j < nrows; ++j) {
        ok = ok && cols[i] < g.dw && rows[j] < g.dh && sample_in_rect(g, w, c, cols[i], rows[j]);
        ++*reads;
      }
  return ok;
}

void check(const Case& c, size_t id, int cb, Tally& tally) {
  jc_geom g;
  jc_geom_init(g, c.H, c.W, c.ncomp, c.hs, c.vs);
  const int nseg = c.meta[JM_NSEG];
  const size_t words = (size_t)g.nblocks * 64;
  const int total = g.mcux * g.mcuy;
  std::vector<int32_t> meta = c.meta;
  meta[JM_OFF] = 0;
  std::vector<int16_t> full(words, 0);
  for (int seg = 0; seg < nseg; ++seg) {
    int s0, s1, m0, m1;
    if (!jc_segment_range(meta.data(), c.width, c.width - JM_SEG, c.len, seg, g, &s0, &s1, &m0, &m1)) exit(2);
    jc_decode_segment(c.data.data(), s0, s1, meta.data(), g, m0, m1, full.data());
  }
  std::vector<uint32_t> rows;
  const long nchunks = jc_chunk_count(0, c.len, cb);
  if (nseg == 1) serial_rows(c.data.data(), c.len, meta.data(), g, cb, rows);
  const long lanes = nseg == 1 ? nchunks : nseg;

  for (size_t bi = 0; bi < c.boxes.size() / 4; ++bi) {
    const int32_t* box = &c.boxes[bi * 4];
    jc_window w;
    bool ok = jc_window_init(g, box[0], box[1], box[2], box[3], w);
    ++tally.windows;
    if (!ok || w.mx0 < 0 || w.my0 < 0 || w.mx1 > g.mcux || w.my1 > g.mcuy || w.mx0 >= w.mx1 || w.my0 >= w.my1) {
      printf("case %zu box %zu: no MCU rectangle inside the frame\n", id, bi);
      ++tally.failed;
      continue;
    }
    const long first = jc_window_first(g, w), last = jc_window_last(g, w);
    int16_t* coef = (int16_t*)calloc(words, 2);                 // exact: a store past the frame is reported
    std::vector<uint8_t> ran(total, 0);                         // MCUs a lane that ran could have written
    int status = 0;
    for (long i = lanes - 1; i >= 0; --i) {
      ++tally.lanes;
      if (nseg == 1) {
        long block, next = (long)total * g.mcu_blocks, after;
        int dc[3], ndc[3];
        const jc_state in = jc_row_unpack(&rows[(size_t)i * JS_ROW_WORDS], jc_chunk_start(c.len, cb, i), c.len, g, &block, dc);
        if (i + 1 < nchunks && !(rows[(size_t)(i + 1) * JS_ROW_WORDS] >> 31)) {
          jc_row_unpack(&rows[(size_t)(i + 1) * JS_ROW_WORDS], jc_chunk_start(c.len, cb, i + 1), c.len, g, &after, ndc);
          next = after;
        }
        if (jc_window_skips_blocks(g, w, block, next)) {
          ++tally.skipped;
          continue;
        }
        for (long m = block / g.mcu_blocks; m < total && m <= next / g.mcu_blocks; ++m) ran[m] = 1;
        status |= jc_chunk_write(c.data.data(), c.len, jc_chunk_end(0, c.len, cb, i), cb, meta.data(), g, in, block, dc,
                                 0, (int)last, coef);
      } else {
        int s0, s1, m0, m1;
        if (!jc_segment_range(meta.data(), c.width, c.width - JM_SEG, c.len, (int)i, g, &s0, &s1, &m0, &m1)) exit(2);
        if (jc_window_skips_mcus(g, w, m0, m1)) {
          ++tally.skipped;
          continue;
        }
        for (long m = m0; m < m1; ++m) ran[m] = 1;
        status |= jc_decode_segment(c.data.data(), s0, s1, meta.data(), g, m0, m1, coef);
      }
    }
    ok = status == 0;
    for (int blk = 0; blk < g.nblocks; ++blk) {
      const long mcu = block_mcu(g, blk);
      const int16_t* a = coef + (size_t)blk * 64;
      bool zero = true;
      for (int k = 0; k < 64; ++k) zero = zero && a[k] == 0;
      if (mcu_in_rect(g, w, mcu)) ok = ok && memcmp(a, &full[(size_t)blk * 64], 128) == 0;
      if (nseg == 1 && mcu >= last) ok = ok && zero;
      if (!ran[mcu]) ok = ok && zero;                           // its chunks or segments were all skipped
    }
    // inverse DCT of the rectangle's blocks alone; every other sample keeps 0x5a
    uint8_t* planes = (uint8_t*)malloc(words);
    memset(planes, 0x5a, words);
    const long nb = jc_window_blocks(g, w);
    std::vector<uint8_t> seen(g.nblocks, 0);
    for (long local = 0; local < nb; ++local) {
      const int blk = jc_window_block(g, w, local);
      if (blk < 0 || blk >= g.nblocks || seen[blk] || !mcu_in_rect(g, w, block_mcu(g, blk))) {
        ok = false;
        break;
      }
      seen[blk] = 1;
      long stride;
      const long at = jc_block_samples(g, blk, &stride);
      jc_idct_block(coef + (size_t)blk * 64, planes + at, stride);
      ++tally.blocks;
    }
    for (int blk = 0; blk < g.nblocks; ++blk) ok = ok && (bool)seen[blk] == mcu_in_rect(g, w, block_mcu(g, blk));
    for (int y = 0; ok && y < w.h; ++y)
      for (int x = 0; x < w.w; ++x) {
        uint8_t px[3];
        jc_pixel(planes, g, w.x0 + x, w.y0 + y, px);
        ok = ok && memcmp(px, &c.rgb[((size_t)(w.y0 + y) * c.W + w.x0 + x) * 3], 3) == 0;
        ok = ok && reads_inside(g, w, w.x0 + x, w.y0 + y, &tally.reads);
        ++tally.pixels;
      }
    if (!ok) {
      printf("case %zu, chunk size %d, box %d %d %d %d: the window differs from the full decode\n", id, cb, box[0],
             box[1], box[2], box[3]);
      ++tally.failed;
    }
    free(coef);
    free(planes);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <cases file> <boxes file>\n", argv[0]);
    return 2;
  }
  std::vector<Case> cases;
  FILE* fb = fopen(argv[2], "rb");
  int32_t bhead[2];
  if (!read_cases(argv[1], true, cases) || !fb || !read_exact(fb, bhead, sizeof bhead) || bhead[0] != 0x4A505742 ||
      bhead[1] != (int32_t)cases.size()) {
    fprintf(stderr, "cannot read %s and %s\n", argv[1], argv[2]);
    return 2;
  }
  for (Case& c : cases) {
    int32_t n;
    if (!read_exact(fb, &n, 4) || n < 1 || n > 4096) return 2;
    c.boxes.resize((size_t)n * 4);
    if (!read_exact(fb, c.boxes.data(), c.boxes.size() * 4)) return 2;
  }
  fclose(fb);

  const int sizes[] = {8, 64};
  Tally t;
  for (int cb : sizes)
    for (size_t i = 0; i < cases.size(); ++i) check(cases[i], i, cb, t);
  printf("%ld windows: %ld entropy lanes, %ld skipped, %ld blocks, %ld pixels equal to the golden crop, %ld reads inside "
         "the rectangle, %ld failed\n", t.windows, t.lanes, t.skipped, t.blocks, t.pixels, t.reads, t.failed);

  // boxes the entry point refuses
  jc_geom g;
  jc_geom_init(g, 40, 56, 3, 2, 2);
  jc_window w;
  const long bad[][4] = {{-1, 0, 1, 1}, {0, -1, 1, 1}, {0, 0, 0, 1}, {0, 0, 1, 0}, {56, 0, 1, 1}, {0, 40, 1, 1},
                         {50, 0, 7, 1}, {0, 30, 1, 11}, {0, 0, 1L << 40, 1}, {1L << 40, 0, 1, 1}};
  int refused = 0;
  for (const auto& b : bad) refused += !jc_window_init(g, b[0], b[1], b[2], b[3], w);
  printf("%d of %zu bad boxes refused\n", refused, sizeof bad / sizeof bad[0]);
  return t.failed || refused != (int)(sizeof bad / sizeof bad[0]) ? 1 : 0;
}
