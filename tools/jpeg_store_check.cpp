// Host check of the store arithmetic of coclr_amd/csrc/jpeg_core.h (jc_store_frame_get, jc_store_segment, jc_row_pack /
// jc_row_unpack), the code that jpeg_store_index_kernel and jpeg_entropy_store_kernel run (tests/test_jpeg_store_cpu.py
// builds this with g++ -fsanitize=address,undefined -fno-sanitize-recover=all and runs it on tests/golden/jpeg_frames.pt):
//
//   jpeg_store_check <cases file>
//
// The cases file is the one tools/jpeg_core_check.cpp reads (tests/_jpeg_cases.py: write_core_check_cases).  Every case
// becomes a store of one frame whose bytes lie behind 4 GiB of nothing (the base is a 64-bit number; only the frame's
// own bytes are allocated, exactly), at chunk sizes 8, 16, 64, 128 and 65536.  For a frame of one restart segment:
//   rows     the kernel's order (tools/jpeg_check.h: relax_windows -- windows of 1024 chunks, cold scans, rounds to the
//            fixed point, prefix sums) packed by jc_row_pack, must equal, word for word, the rows of ONE serial walk
//            over the bytes that notes its state at the first symbol of every chunk (serial_rows, there);
//   decode   every chunk decoded once from its unpacked row, last chunk first, must give jc_decode_segment's
//            coefficients and status;
//   garbage  the rows overwritten with seeded random words, decoded into an exact heap block: every store in bounds.
// For a frame with restart markers every segment found by jc_store_segment must be the one jc_segment_range finds and
// decode alike.  The cases marked `corrupt` are damaged with a seed -- 24 flipped bytes, 5 cuts (the record still
// names the full length: the clamp of jc_store_frame_get), 16 inserted bytes -- and held to the same checks.
// Exit 0 = all held.
#include "jpeg_check.h"

namespace {

constexpr int64_t FAR = 1LL << 32;     // where the frame's bytes lie in the imagined store

struct Tally {
  long frames = 0, rows = 0, segments = 0, garbage = 0, failed = 0;
};

// the rows of one frame as jpeg_store_index_kernel finds them: every chunk's true state packed, and behind the end of
// the real bits, where no window goes, rows that say so
void index_rows(const uint8_t* data, int len, const int32_t* meta, const jc_geom& g, int cb, std::vector<uint32_t>& rows) {
  const long nchunks = jc_chunk_count(0, len, cb);
  const uint32_t total = (uint32_t)((long)g.mcux * g.mcuy * g.mcu_blocks);
  rows.assign((size_t)nchunks * JS_ROW_WORDS, 0xDEADBEEFu);
  const Relaxed r = relax_windows(
      data, 0, len, meta, g, total, cb,
      [&](long chunk, const jc_state& in, const jc_state&, uint32_t block, const uint32_t* dc) {
        jc_row_pack(&rows[(size_t)chunk * JS_ROW_WORDS], in, jc_chunk_start(len, cb, chunk), block, dc);
      });
  const uint32_t none[3] = {0, 0, 0};
  for (long i = r.reached; i < nchunks; ++i)
    jc_row_pack(&rows[(size_t)i * JS_ROW_WORDS], jc_state_past(), 0, total, none);
}

// what a lane of jpeg_entropy_store_kernel does for chunk i of a frame of one segment
int decode_chunk(const jc_store_frame& fr, const jc_geom& g, int cb, const uint32_t* rows, long i, int16_t* coef) {
  long block;
  int dc[3];
  const jc_state in = jc_row_unpack(rows + i * JS_ROW_WORDS, jc_chunk_start(fr.len, cb, i), fr.len, g, &block, dc);
  return jc_chunk_write(fr.bytes, fr.len, jc_chunk_end(0, fr.len, cb, i), cb, fr.meta, g, in, block, dc, 0,
                        g.mcux * g.mcuy, coef);
}

// One case as a one-frame store: `bytes` (the frame's, `have` of them really there) with a record that says `len`.
void check(const Case& c, const uint8_t* bytes, int have, int len, int cb, uint32_t seed, const char* what, size_t id,
           Tally& tally) {
  jc_geom g;
  jc_geom_init(g, c.H, c.W, c.ncomp, c.hs, c.vs);
  uint8_t* heap = (uint8_t*)malloc(have ? have : 1);            // an exact heap block: a read past `have` is reported
  memcpy(heap, bytes, have);
  std::vector<int32_t> tables(JS_TABLE_PAD + JS_TABLE_WORDS);
  memcpy(&tables[JS_TABLE_PAD], &c.meta[JM_QUANT], JS_TABLE_WORDS * 4);
  const int nseg = c.meta[JM_NSEG];
  std::vector<int32_t> segs(c.meta.begin() + JM_SEG, c.meta.begin() + JM_SEG + nseg);
  const int64_t rec[JS_FIELDS] = {FAR, len, c.meta[JM_RI], nseg, 0, 0, 0, jc_geom_pack(c.H, c.W, c.ncomp, c.hs, c.vs)};
  jc_store_frame fr;
  jc_store_frame_get(rec, heap - FAR, FAR + have, tables.data(), 1, fr);     // bytes FAR .. FAR + have of the store
  bool ok = fr.bytes == heap && fr.len == (len < have ? len : have) && fr.H == c.H && fr.W == c.W &&
            fr.ncomp == c.ncomp && fr.hs == c.hs && fr.vs == c.vs && fr.nseg == nseg;
  const size_t words = (size_t)g.nblocks * 64;
  int16_t* serial = (int16_t*)calloc(words, 2);                 // exact too: a store past the frame is reported
  int16_t* store = (int16_t*)calloc(words, 2);
  std::vector<int32_t> meta = c.meta;                           // the descriptor the serial decoder reads
  meta[JM_OFF] = 0;
  meta[JM_LEN] = len;
  ++tally.frames;
  if (ok && nseg == 1) {
    const long nchunks = jc_chunk_count(0, fr.len, cb);
    std::vector<uint32_t> rows, walk;
    index_rows(fr.bytes, fr.len, fr.meta, g, cb, rows);
    serial_rows(fr.bytes, fr.len, fr.meta, g, cb, walk);
    ok = rows == walk && (long)rows.size() == nchunks * JS_ROW_WORDS;
    tally.rows += nchunks;
    const int want = jc_decode_segment(heap, 0, fr.len, meta.data(), g, 0, g.mcux * g.mcuy, serial);
    int got = 0;
    for (long i = nchunks - 1; i >= 0; --i) got |= decode_chunk(fr, g, cb, rows.data(), i, store);
    ok = ok && want == got && memcmp(serial, store, words * 2) == 0;
    for (int round = 0; round < 2; ++round) {                   // rows of random words: in bounds, nothing more is asked
      for (uint32_t& w : rows) w = lcg(seed) << 8 ^ lcg(seed);
      for (long i = 0; i < nchunks; ++i) decode_chunk(fr, g, cb, rows.data(), i, store);
      tally.garbage += nchunks;
    }
  } else if (ok) {
    for (int seg = 0; seg < nseg; ++seg) {
      int s0, s1, m0, m1, t0, t1, n0, n1;
      const bool a = jc_store_segment(fr, segs.data(), nseg, seg, g, &s0, &s1, &m0, &m1);
      const bool b = jc_segment_range(meta.data(), c.width, c.width - JM_SEG, have, seg, g, &t0, &t1, &n0, &n1);
      ok = ok && a && b && s0 == t0 && s1 == t1 && m0 == n0 && m1 == n1;
      if (!ok) break;
      const int want = jc_decode_segment(heap, t0, t1, meta.data(), g, n0, n1, serial);
      const int got = jc_decode_segment(fr.bytes, s0, s1, fr.meta, g, m0, m1, store);
      ok = want == got;
      ++tally.segments;
    }
    int s0, s1, m0, m1;
    ok = ok && memcmp(serial, store, words * 2) == 0 && !jc_store_segment(fr, segs.data(), nseg, nseg, g, &s0, &s1, &m0, &m1) &&
         !jc_store_segment(fr, segs.data(), nseg - 1, 0, g, &s0, &s1, &m0, &m1);
  }
  if (!ok) {
    printf("case %zu, %s, chunk size %d: the store differs from the serial decoder\n", id, what, cb);
    ++tally.failed;
  }
  free(heap);
  free(serial);
  free(store);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  std::vector<Case> cases;
  if (!read_cases(argv[1], false, cases)) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }

  const int sizes[] = {8, 16, 64, 128, 65536};
  Tally clean, damaged;
  for (int cb : sizes)
    for (size_t i = 0; i < cases.size(); ++i)
      check(cases[i], cases[i].data.data(), cases[i].len, cases[i].len, cb, 99u + (uint32_t)i, "as written", i, clean);
  printf("%ld frames x sizes: %ld rows equal to the serial walk, %ld restart segments, %ld garbage rows in bounds, "
         "%ld failed\n", clean.frames, clean.rows, clean.segments, clean.garbage, clean.failed);

  const int damaged_sizes[] = {8, 64, 128};
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    if (!c.corrupt) continue;
    for (int cb : damaged_sizes) {
      uint32_t seed = 777u + (uint32_t)i;
      for (int k = 0; k < 24; ++k) {
        std::vector<uint8_t> d = c.data;
        if (!d.empty()) d[lcg(seed) % d.size()] ^= (uint8_t)(1u << (lcg(seed) & 7));
        check(c, d.data(), c.len, c.len, cb, seed, "flipped", i, damaged);
      }
      for (int k = 0; k < 5; ++k)
        check(c, c.data.data(), (int)((long)c.len * k / 5), c.len, cb, seed, "cut", i, damaged);
      for (int k = 0; k < 16; ++k) {
        std::vector<uint8_t> d = c.data;
        d.insert(d.begin() + lcg(seed) % (d.size() + 1), (uint8_t)lcg(seed));
        check(c, d.data(), c.len + 1, c.len + 1, cb, seed, "inserted", i, damaged);
      }
    }
  }
  printf("%ld damaged frames: %ld rows equal to the serial walk, %ld restart segments, %ld garbage rows in bounds, "
         "%ld failed\n", damaged.frames, damaged.rows, damaged.segments, damaged.garbage, damaged.failed);
  return clean.failed || damaged.failed ? 1 : 0;
}
