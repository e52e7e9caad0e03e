// Host check of the gather arithmetic of coclr_amd/csrc/jpeg_core.h (jc_gather_span, jc_gather_place, jc_gather_end,
// jc_gather_frame_ok, jc_gather_rebase, jc_gather_find, jc_gather_lane), the code that jpeg_store_gather_kernel and the
// host checks of coclr_jpeg_store_gather run (tests/test_jpeg_host_store_cpu.py builds this with
// g++ -fsanitize=address,undefined -fno-sanitize-recover=all and runs it; it takes no arguments and never sees a GPU):
//
//   far      spans, places and rebased records of frames whose store bytes lie at offsets up to 2^40 (nobody pins that
//            much in a test: this is where the 64-bit arithmetic is held against its definition, word by word);
//   copy     for every residue 0..15 of the base and every length 1..49, a store of two frames in an exact heap block
//            is gathered by running every lane of the kernel on the host -- one 16-byte word per lane -- into exact
//            heap arenas filled with 0x5a: every frame's bytes and rows must equal memcpy's, every byte outside the
//            hulls must still be 0x5a, and a lane past the last must copy nothing;
//   garbage  the same lanes over plans of seeded random words: whatever they hold, no word outside the four buffers is
//            touched (the sanitizer sees every access);
//   refuse   jc_gather_frame_ok on records whose bytes or rows leave their arrays.
// Exit 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../coclr_amd/csrc/jpeg_core.h"

namespace {

long failed = 0;

void hold(bool ok, const char* what, long a = 0, long b = 0) {
  if (ok) return;
  if (++failed <= 20) printf("differs: %s (%ld, %ld)\n", what, a, b);
}

uint32_t next(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return s >> 8;
}

// ---- far ------------------------------------------------------------------------------------------------------------
long check_far() {
  const int64_t bases[] = {0, 1, 15, 16, 17, (1LL << 31) - 9, (1LL << 31) + 3, (1LL << 32) - 1, (1LL << 32) + 16,
                           (1LL << 36) + 5, (1LL << 40) - 49, (1LL << 40) - 16, (1LL << 40) - 1, 1LL << 40};
  const int64_t lens[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 65536, 0x7fffffff};
  long n = 0;
  int64_t end = 0, row = 0;
  for (int64_t base : bases)
    for (int64_t len : lens) {
      const int64_t dst = jc_gather_place(end, base);
      jc_span s;
      hold(jc_gather_span(base, len, dst, s), "a span is refused", (long)base, (long)len);
      hold((dst & 15) == (base & 15) && dst >= end && dst - end <= 15, "the place", (long)base, (long)dst);
      // the definition: the 16-byte words that hold a byte of [base, base + len)
      const int64_t first = base / 16, last = len ? (base + len - 1) / 16 : first - 1;
      hold(s.src == first && s.words == last - first + 1 && s.dst == dst / 16, "the hull", (long)base, (long)len);
      hold(s.dst * 16 == end, "hulls follow each other", (long)s.dst, (long)end);
      const int64_t stop = jc_gather_end(s);
      hold(len ? stop % 16 == 0 && stop >= dst + len && stop - (dst + len) <= 15 : stop == end, "the end", (long)stop,
           (long)len);                                          // an empty frame takes no word
      for (int64_t off = 1; off < 16; ++off) hold(!jc_gather_span(base, len, dst + off, s), "an incongruent place");
      const int64_t rec[JS_FIELDS] = {base, len, 7, 1, 3, 11, (1LL << 33) + n, jc_geom_pack(40, 56, 3, 2, 2)};
      int64_t out[JS_FIELDS];
      jc_gather_rebase(rec, dst, row, out);
      for (int k = 0; k < JS_FIELDS; ++k)
        hold(out[k] == (k == JS_BASE ? dst : k == JS_ROW ? row : rec[k]), "a rebased record", k, (long)out[k]);
      int64_t brings = -1;
      hold(jc_gather_frame_ok(rec, base + len, (1LL << 33) + n + jc_chunk_count(0, (int)len, 64), 64, &brings) &&
               brings == jc_chunk_count(0, (int)len, 64),
           "a record inside its arrays is refused", (long)base, (long)len);
      end = stop;
      row += brings;
      ++n;
    }
  jc_span s;
  hold(!jc_gather_span(-1, 1, 15, s) && !jc_gather_span(16, -1, 0, s) && !jc_gather_span(16, 1LL << 31, 0, s) &&
           !jc_gather_span(0, 1, -16, s) && !jc_gather_span((1LL << 62) + 16, 1, 0, s),
       "a range that must be refused");
  return n;
}

// ---- copy -----------------------------------------------------------------------------------------------------------
struct Arena {              // exact heap blocks, 16-byte aligned: an access outside them is reported
  uint8_t* bytes;
  uint8_t* rows;
  int64_t nbytes, nrows;
  Arena(int64_t b, int64_t r) : nbytes(b), nrows(r) {
    bytes = (uint8_t*)aligned_alloc(16, (size_t)(b ? b : 16));
    rows = (uint8_t*)aligned_alloc(16, (size_t)(r ? r * 16 : 16));
    memset(bytes, 0x5a, (size_t)(b ? b : 16));
    memset(rows, 0x5a, (size_t)(r ? r * 16 : 16));
  }
  ~Arena() {
    free(bytes);
    free(rows);
  }
};

// every lane of jpeg_store_gather_kernel, and `extra` lanes behind the last
long run_lanes(const int64_t* plan, long m, int64_t lanes, int extra, const Arena& src, int64_t src_bytes, Arena& dst) {
  long copied = 0;
  for (int64_t id = 0; id < lanes + extra; ++id) {
    bool rows;
    int64_t from, to;
    if (!jc_gather_lane(plan, m, id, (src_bytes + 15) >> 4, src.nrows, dst.nbytes >> 4, dst.nrows, &rows, &from, &to))
      continue;
    hold(from >= 0 && to >= 0, "a negative word", (long)from, (long)to);
    if (from < 0 || to < 0) continue;
    memcpy((rows ? dst.rows : dst.bytes) + to * 16, (rows ? src.rows : src.bytes) + from * 16, 16);
    ++copied;
  }
  return copied;
}

long check_copy(long& garbage) {
  long n = 0;
  uint32_t seed = 0x5EED;
  for (int r = 0; r < 16; ++r)
    for (int len = 1; len <= 49; ++len) {
      // the store: r bytes of another frame, frame A of `len` bytes, frame B; A has chunk rows, B restart markers or rows
      const int lenb = 1 + (len * 7 + r) % 49, cb = 8;
      const int64_t base[2] = {r, r + len}, ln[2] = {len, lenb};
      const int64_t data_bytes = r + len + lenb;
      const int64_t nrow[2] = {jc_chunk_count(0, len, cb), (len & 1) ? 0 : jc_chunk_count(0, lenb, cb)};
      const int64_t srow[2] = {3, 3 + nrow[0]};
      Arena src((data_bytes + 15) & ~15LL, 3 + nrow[0] + nrow[1]);
      for (int64_t i = 0; i < src.nbytes; ++i) src.bytes[i] = (uint8_t)next(seed);
      for (int64_t i = 0; i < src.nrows * 16; ++i) src.rows[i] = (uint8_t)next(seed);
      // the selection: B, then A, or A alone
      for (int order = 0; order < 3; ++order) {
        const int m = order == 2 ? 1 : 2;
        const int pick[2] = {order == 0 ? 1 : 0, order == 0 ? 0 : 1};
        int64_t plan[2 * JG_FIELDS], end = 0, rows = 0, lanes = 0;
        for (int j = 0; j < m; ++j) {
          const int f = pick[j];
          int64_t* p = plan + j * JG_FIELDS;
          jc_span s;
          p[JG_FRAME] = f; p[JG_SRC] = base[f]; p[JG_LEN] = ln[f]; p[JG_DST] = jc_gather_place(end, base[f]);
          p[JG_SRCROW] = srow[f]; p[JG_NROWS] = nrow[f]; p[JG_DSTROW] = rows; p[JG_LANE] = lanes;
          hold(jc_gather_span(p[JG_SRC], p[JG_LEN], p[JG_DST], s), "a span is refused", r, len);
          end = jc_gather_end(s);
          rows += nrow[f];
          lanes += s.words + nrow[f];
        }
        Arena dst(end, rows);
        const long copied = run_lanes(plan, m, lanes, 5, src, data_bytes, dst);
        hold(copied == lanes, "lanes that copied", copied, (long)lanes);
        std::vector<uint8_t> touched((size_t)end, 0);
        for (int j = 0; j < m; ++j) {
          const int64_t* p = plan + j * JG_FIELDS;
          hold(memcmp(dst.bytes + p[JG_DST], src.bytes + p[JG_SRC], (size_t)p[JG_LEN]) == 0, "a frame's bytes", r, len);
          hold(memcmp(dst.rows + p[JG_DSTROW] * 16, src.rows + p[JG_SRCROW] * 16, (size_t)p[JG_NROWS] * 16) == 0,
               "a frame's rows", r, len);
          for (int64_t i = p[JG_DST] & ~15LL; i < ((p[JG_DST] + p[JG_LEN] + 15) & ~15LL); ++i) touched[(size_t)i] = 1;
        }
        for (int64_t i = 0; i < end; ++i) hold(touched[(size_t)i] || dst.bytes[i] == 0x5a, "a byte outside the hulls", r, (long)i);
        // an arena one word short: the lanes that would leave it copy nothing, the others what they copied before
        Arena tight(end - 16, rows ? rows - 1 : 0);
        run_lanes(plan, m, lanes, 0, src, data_bytes, tight);
        hold(end == 16 || memcmp(tight.bytes, dst.bytes, (size_t)(end - 16)) == 0, "a short arena", r, len);
        // plans of random words over the same buffers
        for (int t = 0; t < 8; ++t) {
          int64_t junk[2 * JG_FIELDS];
          for (int64_t& w : junk) {
            const uint32_t kind = next(seed) % 4;
            w = kind == 0 ? (int64_t)(next(seed) % 64) : kind == 1 ? -(int64_t)(next(seed) % 64)
                : kind == 2 ? ((int64_t)(next(seed) & 0x3FFFFF) << 40 | next(seed)) : (int64_t)(next(seed) % 4096) - 64;
          }
          Arena into(end, rows);
          run_lanes(junk, m, lanes + 64, 0, src, data_bytes, into);
          ++garbage;
        }
        ++n;
      }
    }
  return n;
}

// ---- refuse ---------------------------------------------------------------------------------------------------------
long check_refusals() {
  long n = 0;
  const int64_t far = 1LL << 40;
  const auto ok = [&](int64_t base, int64_t len, int64_t nseg, int64_t row, int64_t data_bytes, int64_t nrows) {
    const int64_t rec[JS_FIELDS] = {base, len, 0, nseg, 0, 0, row, 0};
    int64_t brings;
    ++n;
    return jc_gather_frame_ok(rec, data_bytes, nrows, 64, &brings);
  };
  hold(ok(far, 100, 1, 5, far + 100, 7), "the last frame of its arrays");             // 100 bytes: two rows
  hold(!ok(far, 100, 1, 5, far + 99, 7), "bytes that leave the store");
  hold(!ok(far + 1, 100, 1, 5, far + 100, 7), "bytes that leave the store");
  hold(!ok(-1, 100, 1, 5, far, 7), "a negative base");
  hold(!ok(far, -1, 1, 5, far + 100, 7), "a negative length");
  hold(!ok(far, 1LL << 31, 1, 5, far + (1LL << 32), 1LL << 30), "a frame of 2^31 bytes");
  hold(!ok(0, 100, 1, 5, 50, 7), "a store shorter than the frame");
  hold(!ok(far, 100, 1, 6, far + 100, 7), "rows that leave the store");
  hold(!ok(far, 100, 1, -1, far + 100, 7), "a negative row");
  hold(!ok(far, 100, 1, 0, far + 100, 1), "fewer rows than the frame has");
  hold(!ok(far, 100, 0, 5, far + 100, 7), "no segment");
  hold(ok(far, 100, 4, 1LL << 50, far + 100, 1), "restart markers: no rows, whatever the row says");
  hold(ok(far, 0, 1, 6, far, 7) && !ok(far, 0, 1, 7, far, 7), "an empty frame still has a row");
  hold(!ok(far, 100, 1, (int64_t)0x7fffffffffffffffLL, far + 100, 7), "a row at the top of the range");
  return n;
}

}  // namespace

int main() {
  long garbage = 0;
  const long far = check_far();
  const long copies = check_copy(garbage);
  const long refusals = check_refusals();
  printf("gather: %ld far spans, %ld copies, %ld garbage plans, %ld refusals, %ld failed\n", far, copies, garbage,
         refusals, failed);
  return failed ? 1 : 0;
}
