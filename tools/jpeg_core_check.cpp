// Host check of coclr_amd/csrc/jpeg_core.h, the code the gfx950 JPEG kernels run (tests/test_jpeg_cpu.py builds this
// with g++ -fsanitize=address,undefined -fno-sanitize-recover=all, and runs it on tests/golden/jpeg_frames.pt):
//
//   jpeg_core_check <cases file>
//
// The cases file is written by the test from coclr_amd.jpeg.pack; tools/jpeg_check.h has its format and its reader.
// Every case must decode to exactly its expected bytes with status 0.  Cases marked `corrupt` are then decoded again
// damaged -- cut at five points, 32 seeded single-byte overwrites, and once with sixteen one bits at the start of
// the stream, which is no code of any JPEG Huffman table -- in buffers of exactly the sizes the kernels get, so that
// a read or store out of bounds, a signed overflow or a shift out of range ends the program.  The sixteen one bits
// must raise the status flag.  Exit 0 = all held.
#include "jpeg_check.h"

namespace {

// the three stages as the kernels run them, every buffer exactly as large as the entry point asks for
int decode(const Case& c, const std::vector<int32_t>& meta, const uint8_t* data, int len, std::vector<uint8_t>& out) {
  jc_geom g;
  jc_geom_init(g, c.H, c.W, c.ncomp, c.hs, c.vs);
  std::vector<int16_t> coef((size_t)g.nblocks * 64, 0);
  std::vector<uint8_t> planes((size_t)g.nblocks * 64, 0);
  out.assign((size_t)c.H * c.W * 3, 0);
  uint8_t* bytes = (uint8_t*)malloc(len ? len : 1);      // an exact heap block: a read past `len` is reported
  memcpy(bytes, data, len);
  const int maxseg = c.width - JM_SEG;
  int status = 0;
  for (int seg = 0; seg < maxseg; ++seg) {
    int s0, s1, m0, m1;
    if (!jc_segment_range(meta.data(), c.width, maxseg, len, seg, g, &s0, &s1, &m0, &m1)) continue;
    status |= jc_decode_segment(bytes, s0, s1, meta.data(), g, m0, m1, coef.data());
  }
  free(bytes);
  for (int b = 0; b < g.nblocks; ++b) {
    long stride;
    const long at = jc_block_samples(g, b, &stride);
    jc_idct_block(coef.data() + (size_t)b * 64, planes.data() + at, stride);
  }
  for (int y = 0; y < c.H; ++y)
    for (int x = 0; x < c.W; ++x) jc_pixel(planes.data(), g, x, y, out.data() + ((size_t)y * c.W + x) * 3);
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
    return 2;
  }
  std::vector<Case> cases;
  if (!read_cases(argv[1], true, cases)) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  int failed = 0, damaged = 0, flagged = 0;
  for (int i = 0; i < (int)cases.size(); ++i) {
    const Case& c = cases[i];
    std::vector<uint8_t> out;
    const int status = decode(c, c.meta, c.data.data(), c.len, out);
    size_t wrong = 0;
    for (size_t k = 0; k < out.size(); ++k) wrong += out[k] != c.rgb[k];
    if (status != 0 || wrong) {
      printf("case %d (%d x %d, %d components, %dx%d): status %d, %zu bytes differ\n", i, c.W, c.H, c.ncomp, c.hs,
             c.vs, status, wrong);
      ++failed;
    }
    if (!c.corrupt) continue;
    uint32_t seed = 12345u + (uint32_t)i;
    for (int k = 0; k < 5; ++k) {          // cut: the descriptor still names the full length, the buffer is shorter
      const int len = (int)((long)c.len * k / 5);
      flagged += decode(c, c.meta, c.data.data(), len, out) != 0;
      ++damaged;
    }
    for (int k = 0; k < 32; ++k) {
      std::vector<uint8_t> d = c.data;
      if (!d.empty()) d[lcg(seed) % d.size()] = (uint8_t)lcg(seed);
      flagged += decode(c, c.meta, d.data(), c.len, out) != 0;
      ++damaged;
    }
    if (c.len >= 4) {                      // FF 00 FF 00 un-stuffs to sixteen one bits: never a code
      std::vector<uint8_t> d = c.data;
      d[0] = 0xFF; d[1] = 0x00; d[2] = 0xFF; d[3] = 0x00;
      const int st = decode(c, c.meta, d.data(), c.len, out);
      ++damaged;
      if (!(st & JC_BAD_CODE)) {
        printf("case %d: sixteen one bits did not raise the status flag (status %d)\n", i, st);
        ++failed;
      } else {
        ++flagged;
      }
    }
  }
  printf("%d cases, %d failed; %d damaged streams decoded in bounds, %d of them flagged\n", (int)cases.size(), failed,
         damaged, flagged);
  return failed ? 1 : 0;
}
