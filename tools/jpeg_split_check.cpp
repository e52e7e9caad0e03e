// Host check of the chunk arithmetic of coclr_amd/csrc/jpeg_core.h (jc_chunk_scan / jc_chunk_write), the code that
// jpeg_entropy_split_kernel runs (tests/test_jpeg_split_cpu.py builds this with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=all and runs it on tests/golden/jpeg_frames.pt):
//
//   jpeg_split_check <cases file>
//
// The cases file is the one tools/jpeg_core_check.cpp reads (tests/_jpeg_cases.py: write_core_check_cases).  Every
// restart segment of every case is a unit.  A unit is decoded once by jc_decode_segment and once in chunks, in the
// kernel's order (tools/jpeg_check.h: relax_windows -- windows of 1024 chunks, cold scans, rounds to the fixed point,
// prefix sums, carry), every chunk then written from its true state.  Coefficients (a buffer allocated exactly) AND status must be equal byte for
// byte, at chunk sizes 1, 2, 3, 5, 8, 16, 64, 128 and 4096.  The cases marked `corrupt` are then damaged as the
// sibling tool damages them (cut at five points, 32 seeded overwrites, sixteen one bits) and additionally given a
// marker (FF D0) mid-stream and cut inside an FF 00 pair, at chunk sizes 8, 16 and 128: the chunked decode must still
// equal the serial one, in bounds.  Exit 0 = all held.
#include "jpeg_check.h"

namespace {

struct Tally {
  long rounds = 0;                     // the largest round count of any window
  long idle = 0;                       // chunks that owned no symbol start (exit == entry, not past the end)
};

// one segment in chunks, as the kernel's workgroup does it (relax_windows, then the write pass); returns the status bits
int decode_split(const uint8_t* data, int s0, int s1, const int32_t* meta, const jc_geom& g, int m0, int m1,
                 int chunk_bytes, int16_t* coef, Tally& tally) {
  const uint32_t total = (uint32_t)((long)(m1 - m0) * g.mcu_blocks);
  int status = 0;
  const Relaxed r = relax_windows(
      data, s0, s1, meta, g, total, chunk_bytes,
      [&](long chunk, const jc_state& in, const jc_state& out, uint32_t block, const uint32_t* dc) {
        if (in.pos != JC_PAST && same(in, out)) ++tally.idle;
        const int dci[3] = {(int16_t)dc[0], (int16_t)dc[1], (int16_t)dc[2]};
        status |= jc_chunk_write(data, s1, jc_chunk_end(s0, s1, chunk_bytes, chunk), chunk_bytes, meta, g, in,
                                 (long)block, dci, m0, m1, coef);
      });
  for (long rounds : r.rounds)
    if (rounds > tally.rounds) tally.rounds = rounds;
  return status;
}

// all segments of `c` found in `len` bytes of `data`, serially and in chunks; true when coefficients and status agree
bool compare(const Case& c, const uint8_t* data, int len, int chunk_bytes, Tally& tally, int* units,
             int only_seg = -1) {
  jc_geom g;
  jc_geom_init(g, c.H, c.W, c.ncomp, c.hs, c.vs);
  uint8_t* bytes = (uint8_t*)malloc(len ? len : 1);        // an exact heap block: a read past `len` is reported
  memcpy(bytes, data, len);
  const size_t words = (size_t)g.nblocks * 64;
  int16_t* serial = (int16_t*)calloc(words, 2);             // exact too: a store past the frame is reported
  int16_t* split = (int16_t*)calloc(words, 2);
  const int maxseg = c.width - JM_SEG;
  bool ok = true;
  for (int seg = 0; seg < maxseg; ++seg) {
    int s0, s1, m0, m1;
    if (only_seg >= 0 && seg != only_seg) continue;
    if (!jc_segment_range(c.meta.data(), c.width, maxseg, len, seg, g, &s0, &s1, &m0, &m1)) continue;
    memset(serial, 0, words * 2);
    memset(split, 0, words * 2);
    const int want = jc_decode_segment(bytes, s0, s1, c.meta.data(), g, m0, m1, serial);
    const int got = decode_split(bytes, s0, s1, c.meta.data(), g, m0, m1, chunk_bytes, split, tally);
    if (units) ++*units;
    if (want != got || memcmp(serial, split, words * 2) != 0) ok = false;
  }
  free(bytes);
  free(serial);
  free(split);
  return ok;
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

  const int sizes[] = {1, 2, 3, 5, 8, 16, 64, 128, 4096};
  int units = 0, failed = 0;
  for (int cb : sizes) {
    Tally tally;
    for (size_t i = 0; i < cases.size(); ++i) {
      const Case& c = cases[i];
      const int segs = c.width - JM_SEG;
      for (int seg = 0; seg < segs; ++seg) {
        int n = 0;
        const bool ok = compare(c, c.data.data(), c.len, cb, tally, &n, seg);
        units += n;
        if (n && !ok) {
          printf("case %zu segment %d at chunk size %d: differs from the serial decoder\n", i, seg, cb);
          ++failed;
        }
      }
    }
    printf("chunk size %d: at most %ld rounds, %ld chunks owned no symbol start\n", cb, tally.rounds, tally.idle);
  }
  printf("%d units x sizes, %d failed\n", units, failed);

  const int damaged_sizes[] = {8, 16, 128};
  int damaged = 0, unequal = 0;
  Tally ignored;
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    if (!c.corrupt) continue;
    for (int cb : damaged_sizes) {
      auto check = [&](const std::vector<uint8_t>& d, int len, const char* what) {
        ++damaged;
        if (!compare(c, d.data(), len, cb, ignored, nullptr)) {
          printf("case %zu, %s, chunk size %d: differs from the serial decoder\n", i, what, cb);
          ++unequal;
        }
      };
      uint32_t seed = 12345u + (uint32_t)i;
      for (int k = 0; k < 5; ++k)          // cut: the descriptor still names the full length, the buffer is shorter
        check(c.data, (int)((long)c.len * k / 5), "cut");
      for (int k = 0; k < 32; ++k) {
        std::vector<uint8_t> d = c.data;
        if (!d.empty()) d[lcg(seed) % d.size()] = (uint8_t)lcg(seed);
        check(d, c.len, "overwritten");
      }
      if (c.len >= 4) {                    // FF 00 FF 00 un-stuffs to sixteen one bits: never a code
        std::vector<uint8_t> d = c.data;
        d[0] = 0xFF; d[1] = 0x00; d[2] = 0xFF; d[3] = 0x00;
        check(d, c.len, "sixteen one bits");
      }
      if (c.len >= 4) {                    // a marker mid-stream: only zero bits behind it
        std::vector<uint8_t> d = c.data;
        d[c.len / 2] = 0xFF; d[c.len / 2 + 1] = 0xD0;
        check(d, c.len, "planted marker");
      }
      if (c.len >= 4) {                    // cut inside an FF 00 pair: the FF is the buffer's last byte
        std::vector<uint8_t> d = c.data;
        const int at = c.len / 3;
        d[at] = 0xFF; d[at + 1] = 0x00;
        check(d, at + 1, "cut inside FF 00");
      }
    }
  }
  printf("%d damaged streams equal to the serial decoder\n", damaged - unequal);
  return failed || unequal ? 1 : 0;
}
