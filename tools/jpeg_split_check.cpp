// Host check of the chunk arithmetic of coclr_amd/csrc/jpeg_core.h (jc_chunk_scan / jc_chunk_write), the code that
// jpeg_entropy_split_kernel runs (tests/test_jpeg_split_cpu.py builds this with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=all and runs it on tests/golden/jpeg_frames.pt):
//
//   jpeg_split_check <cases file>
//
// The cases file is the one tools/jpeg_core_check.cpp reads (tests/_jpeg_cases.py: write_core_check_cases).  Every
// restart segment of every case is a unit.  A unit is decoded once by jc_decode_segment and once in chunks, in the
// kernel's order: windows of 1024 chunks; in a window cold scans, then rounds in which ALL chunks read the previous
// round's exits and those whose entry changed scan again, until a round changes nothing; a prefix sum of block
// counts and DC sums; the write pass.  Coefficients (a buffer allocated exactly) AND status must be equal byte for
// byte, at chunk sizes 1, 2, 3, 5, 8, 16, 64, 128 and 4096.  The cases marked `corrupt` are then damaged as the
// sibling tool damages them (cut at five points, 32 seeded overwrites, sixteen one bits) and additionally given a
// marker (FF D0) mid-stream and cut inside an FF 00 pair, at chunk sizes 8, 16 and 128: the chunked decode must still
// equal the serial one, in bounds.  Exit 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../coclr_amd/csrc/jpeg_core.h"

namespace {

constexpr int LANES = 1024;            // the kernel's largest workgroup: chunks per window

struct Case {
  int H, W, ncomp, hs, vs, width, len, corrupt;
  std::vector<int32_t> meta;
  std::vector<uint8_t> data;
};

struct Tally {
  long rounds = 0;                     // the largest round count of any window
  long idle = 0;                       // chunks that owned no symbol start (exit == entry, not past the end)
};

bool same(const jc_state& a, const jc_state& b) { return a.pos == b.pos && jc_state_word(a) == jc_state_word(b); }

// one segment in chunks, as the kernel's workgroup does it; returns the status bits
int decode_split(const uint8_t* data, int s0, int s1, const int32_t* meta, const jc_geom& g, int m0, int m1,
                 int chunk_bytes, int16_t* coef, Tally& tally) {
  const long nchunks = jc_chunk_count(s0, s1, chunk_bytes);
  const uint32_t total = (uint32_t)((long)(m1 - m0) * g.mcu_blocks);
  jc_state first = jc_state_make(s0, 0, 0, 0);
  uint32_t block0 = 0, dc0[3] = {0, 0, 0};
  int status = 0;
  std::vector<jc_state> in(LANES), out(LANES), prev(LANES);
  std::vector<int> blocks(LANES);
  std::vector<uint32_t> dcs((size_t)LANES * 3);
  for (long w0 = 0; w0 < nchunks; w0 += LANES) {
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
    if (rounds > tally.rounds) tally.rounds = rounds;
    uint32_t block = block0, dc[3] = {dc0[0], dc0[1], dc0[2]};
    for (int t = 0; t < n; ++t) {
      if (in[t].pos != JC_PAST && same(in[t], out[t])) ++tally.idle;
      const int dci[3] = {(int16_t)dc[0], (int16_t)dc[1], (int16_t)dc[2]};
      status |= jc_chunk_write(data, s1, jc_chunk_end(s0, s1, chunk_bytes, w0 + t), chunk_bytes, meta, g, in[t],
                               (long)block, dci, m0, m1, coef);
      block = jc_blocks_add(block, (uint32_t)blocks[t], total);
      for (int c = 0; c < 3; ++c) dc[c] += dcs[(size_t)t * 3 + c];
    }
    first = out[n - 1];
    block0 = block;
    for (int c = 0; c < 3; ++c) dc0[c] = dc[c];
  }
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

uint32_t lcg(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return s >> 8;
}

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  int32_t head[2];
  if (!f || !read_exact(f, head, sizeof head) || head[0] != 0x4A504731 || head[1] < 1) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<Case> cases(head[1]);
  for (Case& c : cases) {
    int32_t h[8];
    if (!read_exact(f, h, sizeof h)) return 2;
    c.H = h[0]; c.W = h[1]; c.ncomp = h[2]; c.hs = h[3]; c.vs = h[4]; c.width = h[5]; c.len = h[6]; c.corrupt = h[7];
    if (c.H < 1 || c.W < 1 || c.H > 8192 || c.W > 8192 || c.width <= JM_SEG || c.width > (1 << 20) || c.len < 0)
      return 2;
    c.meta.resize(c.width);
    c.data.resize(c.len);
    if (!read_exact(f, c.meta.data(), (size_t)c.width * 4) || !read_exact(f, c.data.data(), c.len) ||
        fseek(f, (long)c.H * c.W * 3, SEEK_CUR) != 0)
      return 2;
    c.meta[JM_OFF] = 0;                    // the case's bytes stand alone
  }
  fclose(f);

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
