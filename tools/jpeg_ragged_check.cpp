// Host check of the ragged addressing of coclr_amd/csrc/jpeg_core.h (jc_find_frame, jc_ragged_frame), the code the
// gfx950 kernels of coclr_jpeg_decode_ragged run (tests/test_ragged_cpu.py builds this with
// g++ -fsanitize=address,undefined -fno-sanitize-recover=all and runs it on tests/golden/jpeg_frames.pt):
//
//   jpeg_ragged_check <cases file>
//
// The cases file is the one of tools/jpeg_core_check.cpp.  Two parts:
//   search  jc_find_frame over prefix arrays of frames of one lane, of many equal frames and of mixed counts: the
//           first and the last lane of every frame, every lane of the small ones, and ids past the end (which land in
//           the last frame with a local index outside its count, as the kernels turn them away).
//   batch   ALL cases as ONE mixed batch, laid out as coclr_amd.jpeg.decode_ragged lays it out (coefficient blocks one
//           frame after the other, output frames 16-byte aligned in a buffer filled with 0x5a), decoded lane by lane
//           the way the kernels do: entropy per frame, then one lane per block and one per 16-pixel row group, each
//           finding its frame by the search.  Every frame must equal its expected bytes and every byte between and
//           behind the frames must still be 0x5a.  All buffers are exact heap blocks, so a store outside is reported.
// Exit 0 = all held.
#include "jpeg_check.h"

namespace {

constexpr long kMaxSide = 8192;

int check_prefix(const std::vector<int64_t>& count, const char* what) {
  const long F = (long)count.size();
  std::vector<int64_t> prefix(F + 1, 0);
  for (long f = 0; f < F; ++f) prefix[f + 1] = prefix[f] + count[f];
  int bad = 0;
  for (long f = 0; f < F; ++f) {
    const long ids[4] = {(long)prefix[f], (long)prefix[f + 1] - 1, (long)prefix[f] + count[f] / 2, (long)prefix[f] + 1};
    for (int k = 0; k < 4; ++k) {
      if (ids[k] < prefix[f] || ids[k] >= prefix[f + 1]) continue;
      if (jc_find_frame(prefix.data(), F, ids[k]) != f) ++bad;
    }
    if (count[f] <= 64)
      for (long id = prefix[f]; id < prefix[f + 1]; ++id) bad += jc_find_frame(prefix.data(), F, id) != f;
  }
  for (long past = 0; past < 3; ++past) {            // behind the end: the last frame, and a local index outside it
    const long id = prefix[F] + past * 1000;
    const long f = jc_find_frame(prefix.data(), F, id);
    if (f != F - 1 || id - prefix[f] < count[f]) ++bad;
  }
  if (jc_find_frame(prefix.data(), F, -5) != 0) ++bad;                 // and in front of it: frame 0, local < 0
  if (bad) printf("search (%s): %d wrong answers\n", what, bad);
  return bad;
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

  // ---- search -------------------------------------------------------------------------------------------------------
  int searched = 0, wrong = 0;
  {
    std::vector<int64_t> ones(300, 1), equal(1000, 1800), single(1, 7), mixed;
    uint32_t s = 99u;
    for (int i = 0; i < 257; ++i) {
      const uint32_t v = lcg(s);
      mixed.push_back(i % 5 == 0 ? 1 : 1 + v % 5000);
    }
    wrong += check_prefix(ones, "frames of one lane");
    wrong += check_prefix(equal, "many equal frames");
    wrong += check_prefix(single, "one frame");
    wrong += check_prefix(mixed, "mixed");
    searched = 4;
  }

  // ---- the mixed batch ----------------------------------------------------------------------------------------------
  const long F = (long)cases.size();
  std::vector<int64_t> tab((size_t)F * JR_FIELDS, 0), pblocks(F + 1, 0), prows(F + 1, 0);
  long obytes = 0;
  for (long i = 0; i < F; ++i) {
    const Case& c = cases[i];
    jc_geom g;
    jc_geom_init(g, c.H, c.W, c.ncomp, c.hs, c.vs);
    int64_t* t = tab.data() + i * JR_FIELDS;
    t[JR_H] = c.H; t[JR_W] = c.W; t[JR_NCOMP] = c.ncomp; t[JR_HS] = c.hs; t[JR_VS] = c.vs;
    t[JR_CBLOCK] = pblocks[i];
    t[JR_OBYTE] = obytes;
    pblocks[i + 1] = pblocks[i] + g.nblocks;
    prows[i + 1] = prows[i] + jc_row_groups(g);
    obytes = (obytes + (long)c.H * c.W * 3 + 15) & ~15L;
  }
  const long coef_blocks = pblocks[F], out_bytes = obytes;
  int16_t* coef = (int16_t*)calloc((size_t)coef_blocks * 64, 2);
  uint8_t* planes = (uint8_t*)calloc((size_t)coef_blocks * 64, 1);
  uint8_t* out = (uint8_t*)malloc((size_t)out_bytes);
  if (!coef || !planes || !out) return 2;
  memset(out, 0x5a, (size_t)out_bytes);
  int status = 0, skipped = 0;
  for (long i = 0; i < F; ++i) {                       // entropy: a lane per (frame, segment)
    const Case& c = cases[i];
    jc_geom g;
    long cb, ob;
    if (!jc_ragged_frame(tab.data(), i, coef_blocks, out_bytes, kMaxSide, g, &cb, &ob)) { ++skipped; continue; }
    const int maxseg = c.width - JM_SEG;
    for (int seg = 0; seg < maxseg; ++seg) {
      int s0, s1, m0, m1;
      if (!jc_segment_range(c.meta.data(), c.width, maxseg, c.len, seg, g, &s0, &s1, &m0, &m1)) continue;
      status |= jc_decode_segment(c.data.data(), s0, s1, c.meta.data(), g, m0, m1, coef + cb * 64);
    }
  }
  for (long id = 0; id < pblocks[F] + 300; ++id) {     // inverse DCT: a lane per block, and lanes past the end
    const long fr = jc_find_frame(pblocks.data(), F, id);
    jc_geom g;
    long cb, ob;
    if (!jc_ragged_frame(tab.data(), fr, coef_blocks, out_bytes, kMaxSide, g, &cb, &ob)) continue;
    const long local = id - pblocks[fr];
    if (local < 0 || local >= g.nblocks) continue;
    long stride;
    const long at = jc_block_samples(g, (int)local, &stride);
    jc_idct_block(coef + (cb + local) * 64, planes + cb * 64 + at, stride);
  }
  for (long id = 0; id < prows[F] + 300; ++id) {       // colour: a lane per 16 pixels of a row
    const long fr = jc_find_frame(prows.data(), F, id);
    jc_geom g;
    long cb, ob;
    if (!jc_ragged_frame(tab.data(), fr, coef_blocks, out_bytes, kMaxSide, g, &cb, &ob)) continue;
    const long local = id - prows[fr];
    if (local < 0 || local >= jc_row_groups(g)) continue;
    const int groups = (g.W + 15) / 16;
    const int xg = (int)(local % groups), y = (int)(local / groups);
    const int nx = g.W - xg * 16 < 16 ? g.W - xg * 16 : 16;
    for (int k = 0; k < nx; ++k)
      jc_pixel(planes + cb * 64, g, xg * 16 + k, y, out + ob + ((long)y * g.W + xg * 16 + k) * 3);
  }
  int failed = 0;
  long gap_bytes = 0, gap_wrong = 0, at = 0;
  for (long i = 0; i < F; ++i) {
    const Case& c = cases[i];
    const long ob = tab[i * JR_FIELDS + JR_OBYTE];
    for (; at < ob; ++at) { ++gap_bytes; gap_wrong += out[at] != 0x5a; }
    size_t differ = 0;
    for (size_t k = 0; k < c.rgb.size(); ++k) differ += out[ob + k] != c.rgb[k];
    if (differ) {
      printf("frame %ld (%d x %d, %d components, %dx%d): %zu bytes differ\n", i, c.W, c.H, c.ncomp, c.hs, c.vs, differ);
      ++failed;
    }
    at = ob + (long)c.rgb.size();
  }
  for (; at < out_bytes; ++at) { ++gap_bytes; gap_wrong += out[at] != 0x5a; }
  // a table the kernels must turn away: a frame whose storage leaves the buffers, and a geometry they do not take
  {
    std::vector<int64_t> bad(tab.begin(), tab.begin() + JR_FIELDS);
    jc_geom g;
    long cb, ob;
    int held = 0;
    bad[JR_CBLOCK] = coef_blocks;
    held += !jc_ragged_frame(bad.data(), 0, coef_blocks, out_bytes, kMaxSide, g, &cb, &ob);
    bad[JR_CBLOCK] = -1;
    held += !jc_ragged_frame(bad.data(), 0, coef_blocks, out_bytes, kMaxSide, g, &cb, &ob);
    bad[JR_CBLOCK] = 0;
    bad[JR_OBYTE] = out_bytes - 1;
    held += !jc_ragged_frame(bad.data(), 0, coef_blocks, out_bytes, kMaxSide, g, &cb, &ob);
    bad[JR_OBYTE] = 0;
    bad[JR_HS] = 4;
    held += !jc_ragged_frame(bad.data(), 0, coef_blocks, out_bytes, kMaxSide, g, &cb, &ob);
    bad[JR_HS] = tab[JR_HS];
    bad[JR_W] = (int64_t)1 << 40;
    held += !jc_ragged_frame(bad.data(), 0, coef_blocks, out_bytes, kMaxSide, g, &cb, &ob);
    if (held != 5) {
      printf("jc_ragged_frame let %d of 5 bad tables through\n", 5 - held);
      ++failed;
    }
  }
  free(coef);
  free(planes);
  free(out);
  printf("%d searches, %d wrong; %ld frames in one batch, %d failed, %d skipped, status %d; %ld bytes between frames, "
         "%ld touched\n", searched, wrong, F, failed, skipped, status, gap_bytes, gap_wrong);
  return (wrong || failed || skipped || status || gap_wrong) ? 1 : 0;
}
