// Host check of the SHARDED gather arithmetic of coclr_amd/csrc/jpeg_core.h (jc_gather_lane_from, jc_gather_order_ok,
// and through them jc_gather_span, jc_gather_place, jc_gather_end, jc_gather_find), the code that
// jpeg_store_gather_kernel<shard_sources> and the host checks of coclr_jpeg_store_gather_shards run
// (tests/test_jpeg_shard_cpu.py builds this with g++ -fsanitize=address,undefined -fno-sanitize-recover=all and runs it;
// it takes no arguments and never sees a GPU).  tools/jpeg_gather_check.cpp holds the one-source case.
//
//   copy     for every residue 0..15 and every length 1..49, a dataset of two frames per shard over 1, 2, 3 and 8 shards
//            (and 8 with one shard EMPTY), every shard an exact heap block of its own with its bytes starting at another
//            residue, is gathered by running every lane of the kernel on the host -- one 16-byte word per lane -- into
//            exact heap arenas filled with 0x5a: every frame's bytes and rows must equal memcpy's from its OWN shard,
//            every byte outside the hulls must still be 0x5a, and lanes past the last must copy nothing;
//   garbage  the same lanes over plans AND shard columns of seeded random words, and over the true plan with a random
//            shard column: whatever they hold, no word outside the buffers is touched (the sanitizer sees every access)
//            and no source outside the table is named;
//   far      lanes of frames whose shard bytes lie at offsets up to 2^40, in a shard other than the first: the word
//            addresses against their definition (nothing is copied: nobody allocates that much);
//   order    jc_gather_order_ok on columns that are, and are not, ordered by (shard, frame).
// The property "in bounds whatever the device data holds" is proved HERE, on the host; no GPU test feeds the kernel a
// corrupt plan.  Exit 0 = all held.
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

struct Block {              // exact heap blocks, 16-byte aligned: an access outside them is reported
  uint8_t* bytes;
  uint8_t* rows;
  int64_t nbytes, nrows;
  Block(int64_t b, int64_t r, int fill = 0x5a) : nbytes(b), nrows(r) {
    bytes = (uint8_t*)aligned_alloc(16, (size_t)(b ? b : 16));
    rows = (uint8_t*)aligned_alloc(16, (size_t)(r ? r * 16 : 16));
    memset(bytes, fill, (size_t)(b ? b : 16));
    memset(rows, fill, (size_t)(r ? r * 16 : 16));
  }
  Block(const Block&) = delete;
  ~Block() {
    free(bytes);
    free(rows);
  }
};

// the kernel's table entry: the members of jc_gather_size and the two pointers
struct Source {
  const uint8_t* data;
  int64_t words;
  const uint8_t* rows;
  int64_t nrows;
};

// every lane of jpeg_store_gather_kernel<shard_sources>, and `extra` lanes behind the last
long run_lanes(const int64_t* plan, const int64_t* shard, long m, int64_t lanes, int extra, const Source* srcs,
               int nshards, Block& dst) {
  long copied = 0;
  for (int64_t id = 0; id < lanes + extra; ++id) {
    bool rows;
    int64_t which = -1, from, to;
    if (!jc_gather_lane_from(plan, shard, m, id, srcs, nshards, dst.nbytes >> 4, dst.nrows, &which, &rows, &from, &to))
      continue;
    hold(which >= 0 && which < nshards && from >= 0 && to >= 0, "a source or word outside", (long)which, (long)from);
    if (which < 0 || which >= nshards || from < 0 || to < 0) continue;
    memcpy((rows ? dst.rows : dst.bytes) + to * 16, (rows ? srcs[which].rows : srcs[which].data) + from * 16, 16);
    ++copied;
  }
  return copied;
}

int64_t junk_word(uint32_t& seed) {
  const uint32_t kind = next(seed) % 4;
  return kind == 0 ? (int64_t)(next(seed) % 64) : kind == 1 ? -(int64_t)(next(seed) % 64)
         : kind == 2 ? ((int64_t)(next(seed) & 0x3FFFFF) << 40 | next(seed)) : (int64_t)(next(seed) % 4096) - 64;
}

// ---- copy, garbage --------------------------------------------------------------------------------------------------
long check_copy(long& garbage) {
  long n = 0;
  uint32_t seed = 0x5EED;
  const int configs[5][2] = {{1, -1}, {2, -1}, {3, -1}, {8, -1}, {8, 5}};      // shards, the empty one
  for (int r = 0; r < 16; ++r)
    for (int len = 1; len <= 49; ++len)
      for (const auto& cfg : configs) {
        const int nshards = cfg[0], empty = cfg[1], cb = 8;
        // shard k: (r + 5 k) % 16 bytes of another frame, frame A of `len + k` bytes (1..56), frame B; A has chunk rows,
        // B restart markers (no rows) in odd shards
        std::vector<Block*> blocks;
        Source srcs[JG_MAX_SHARDS];
        int64_t base[JG_MAX_SHARDS][2], ln[JG_MAX_SHARDS][2], nrow[JG_MAX_SHARDS][2], srow[JG_MAX_SHARDS][2];
        for (int k = 0; k < nshards; ++k) {
          const int lead = (r + 5 * k) % 16, la = k == empty ? 0 : len + k, lb = k == empty ? 0 : 1 + (len * 7 + r + k) % 49;
          base[k][0] = lead; base[k][1] = lead + la; ln[k][0] = la; ln[k][1] = lb;
          nrow[k][0] = k == empty ? 0 : jc_chunk_count(0, la, cb);
          nrow[k][1] = (k == empty || (k & 1)) ? 0 : jc_chunk_count(0, lb, cb);
          srow[k][0] = k; srow[k][1] = k + nrow[k][0];
          const int64_t data_bytes = lead + la + lb;
          Block* b = new Block((data_bytes + 15) & ~15LL, k + nrow[k][0] + nrow[k][1]);
          for (int64_t i = 0; i < b->nbytes; ++i) b->bytes[i] = (uint8_t)next(seed);
          for (int64_t i = 0; i < b->nrows * 16; ++i) b->rows[i] = (uint8_t)next(seed);
          blocks.push_back(b);
          srcs[k] = {b->bytes, (data_bytes + 15) >> 4, b->rows, b->nrows};
        }
        // the selection: both frames of every shard that has any, but only B of shard 0 when len is odd
        int64_t plan[2 * JG_MAX_SHARDS * JG_FIELDS], shard[2 * JG_MAX_SHARDS], end = 0, rows = 0, lanes = 0;
        long m = 0;
        for (int k = 0; k < nshards; ++k)
          for (int f = 0; f < 2; ++f) {
            if (k == empty || (k == 0 && f == 0 && (len & 1) && nshards > 1)) continue;
            int64_t* p = plan + m * JG_FIELDS;
            jc_span s;
            p[JG_FRAME] = f; p[JG_SRC] = base[k][f]; p[JG_LEN] = ln[k][f]; p[JG_DST] = jc_gather_place(end, base[k][f]);
            p[JG_SRCROW] = srow[k][f]; p[JG_NROWS] = nrow[k][f]; p[JG_DSTROW] = rows; p[JG_LANE] = lanes;
            shard[m] = k;
            hold(jc_gather_span(p[JG_SRC], p[JG_LEN], p[JG_DST], s), "a span is refused", r, len);
            hold(jc_gather_order_ok(plan, shard, m, nshards), "an ordered row is refused", k, f);
            end = jc_gather_end(s);
            rows += nrow[k][f];
            lanes += s.words + nrow[k][f];
            ++m;
          }
        Block dst(end, rows);
        const long copied = run_lanes(plan, shard, m, lanes, 5, srcs, nshards, dst);
        hold(copied == lanes, "lanes that copied", copied, (long)lanes);
        std::vector<uint8_t> touched((size_t)end, 0);
        for (long j = 0; j < m; ++j) {
          const int64_t* p = plan + j * JG_FIELDS;
          const Source& s = srcs[shard[j]];
          hold(memcmp(dst.bytes + p[JG_DST], s.data + p[JG_SRC], (size_t)p[JG_LEN]) == 0, "a frame's bytes", r, len);
          hold(memcmp(dst.rows + p[JG_DSTROW] * 16, s.rows + p[JG_SRCROW] * 16, (size_t)p[JG_NROWS] * 16) == 0,
               "a frame's rows", r, len);
          for (int64_t i = p[JG_DST] & ~15LL; i < ((p[JG_DST] + p[JG_LEN] + 15) & ~15LL); ++i) touched[(size_t)i] = 1;
        }
        for (int64_t i = 0; i < end; ++i)
          hold(touched[(size_t)i] || dst.bytes[i] == 0x5a, "a byte outside the hulls", r, (long)i);
        // an arena one word short: the lanes that would leave it copy nothing, the others what they copied before
        Block tight(end - 16, rows ? rows - 1 : 0);
        run_lanes(plan, shard, m, lanes, 0, srcs, nshards, tight);
        hold(end == 16 || memcmp(tight.bytes, dst.bytes, (size_t)(end - 16)) == 0, "a short arena", r, len);
        // a shard index outside the table copies nothing, whatever the row holds
        {
          std::vector<int64_t> out(shard, shard + m);
          for (int64_t& w : out) w = (&w - out.data()) & 1 ? nshards : -1;
          Block into(end, rows);
          hold(run_lanes(plan, out.data(), m, lanes, 0, srcs, nshards, into) == 0, "a source outside the table", r, len);
        }
        // plans and shard columns of random words over the same buffers; then the true plan, a random column
        for (int t = 0; t < 16; ++t) {
          int64_t junk[2 * JG_MAX_SHARDS * JG_FIELDS], column[2 * JG_MAX_SHARDS];
          for (long i = 0; i < m * JG_FIELDS; ++i) junk[i] = t < 8 ? junk_word(seed) : plan[i];
          for (long i = 0; i < m; ++i) column[i] = (next(seed) & 1) ? (int64_t)(next(seed) % 10) - 1 : junk_word(seed);
          Block into(end, rows);
          run_lanes(junk, column, m, lanes + 64, 0, srcs, nshards, into);
          ++garbage;
        }
        for (Block* b : blocks) delete b;
        ++n;
      }
  return n;
}

// ---- far ------------------------------------------------------------------------------------------------------------
long check_far() {
  const int64_t bases[] = {0, 1, 15, 16, 17, (1LL << 31) - 9, (1LL << 31) + 3, (1LL << 32) - 1, (1LL << 32) + 16,
                           (1LL << 36) + 5, (1LL << 40) - 49, (1LL << 40) - 16, (1LL << 40) - 1, 1LL << 40};
  const int64_t lens[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 65536, 0x7fffffff};
  long n = 0;
  for (int64_t base : bases)
    for (int64_t len : lens) {
      // shard 0 is tiny; the frame lies in shard `k`, whose size is exactly the frame's end
      const int k = 1 + (int)(n % 7);
      jc_gather_size srcs[JG_MAX_SHARDS];
      for (auto& s : srcs) s = {1, 1};
      const int64_t row = (1LL << 33) + n, nrows = jc_chunk_count(0, (int)len, 64);
      srcs[k] = {(base + len + 15) >> 4, row + nrows};
      const int64_t end = 48, dst = jc_gather_place(end, base);
      const int64_t plan[2 * JG_FIELDS] = {0, 0, 16, 0, 0, 1, 0, 0, /* row 1 */ 5, base, len, dst, row, nrows, 1, 2};
      const int64_t shard[2] = {0, k};
      const int64_t words = len ? ((base + len + 15) >> 4) - (base >> 4) : 0;
      const int64_t probes[] = {0, words / 2, words - 1, words, words + nrows - 1};
      for (int64_t local : probes) {
        if (local < 0 || local >= words + nrows) continue;
        bool rows;
        int64_t which, from, to;
        const bool ok = jc_gather_lane_from(plan, shard, 2, 2 + local, srcs, 8, (1LL << 41), (1LL << 41), &which, &rows,
                                            &from, &to);
        const bool is_row = local >= words;
        hold(ok && which == k && rows == is_row, "a far lane", (long)base, (long)local);
        hold(from == (is_row ? row + local - words : (base >> 4) + local), "a far source word", (long)base, (long)from);
        hold(to == (is_row ? 1 + local - words : (dst >> 4) + local), "a far arena word", (long)base, (long)to);
      }
      // one word, or one row, short of the frame: the last lanes copy nothing; held against shard 0 nothing fits
      bool rows;
      int64_t which, from, to;
      if (words) {
        srcs[k].words -= 1;
        hold(!jc_gather_lane_from(plan, shard, 2, 2 + words - 1, srcs, 8, 1LL << 41, 1LL << 41, &which, &rows, &from, &to),
             "a word past its shard", (long)base, (long)len);
        srcs[k].words += 1;
      }
      srcs[k].nrows -= 1;
      hold(!jc_gather_lane_from(plan, shard, 2, 2 + words + nrows - 1, srcs, 8, 1LL << 41, 1LL << 41, &which, &rows, &from,
                                &to),
           "a row past its shard", (long)base, (long)len);
      const int64_t wrong[2] = {0, 0};
      hold(base < 16 || !words ||
               !jc_gather_lane_from(plan, wrong, 2, 2, srcs, 8, 1LL << 41, 1LL << 41, &which, &rows, &from, &to),
           "a far word held against another shard's size", (long)base, (long)len);
      ++n;
    }
  return n;
}

// ---- order ----------------------------------------------------------------------------------------------------------
long check_order() {
  long n = 0;
  const auto ok = [&](std::vector<int64_t> shard, std::vector<int64_t> frame, int nshards) {
    std::vector<int64_t> plan(frame.size() * JG_FIELDS, 0);
    for (size_t j = 0; j < frame.size(); ++j) plan[j * JG_FIELDS + JG_FRAME] = frame[j];
    ++n;
    for (size_t j = 0; j < frame.size(); ++j)
      if (!jc_gather_order_ok(plan.data(), shard.data(), (long)j, nshards)) return false;
    return true;
  };
  hold(ok({0}, {0}, 1), "one row");
  hold(ok({0, 0, 1, 1, 7}, {0, 5, 0, 9, 3}, 8), "ordered by (shard, frame)");
  hold(ok({2, 5}, {1LL << 40, 0}, 8), "a later shard starts again");
  hold(!ok({0, 0}, {5, 5}, 8), "a frame twice");
  hold(!ok({0, 0}, {5, 4}, 8), "frames that decrease inside a shard");
  hold(!ok({1, 0}, {0, 1}, 8), "shards that decrease");
  hold(!ok({0, 8}, {0, 0}, 8), "a shard of nshards");
  hold(!ok({0, 3}, {0, 0}, 3), "a shard of nshards");
  hold(!ok({-1}, {0}, 8), "a negative shard");
  hold(!ok({0}, {-1}, 8), "a negative frame");
  hold(!ok({0, 1LL << 40}, {0, 0}, 8), "a shard of 2^40");
  hold(!ok({0, 1, 1, 0}, {0, 0, 1, 1}, 8), "a late return to an earlier shard");
  return n;
}

}  // namespace

int main() {
  long garbage = 0;
  const long copies = check_copy(garbage);
  const long far = check_far();
  const long orders = check_order();
  printf("shard gather: %ld copies, %ld garbage plans and columns, %ld far frames, %ld orders, %ld failed\n", copies,
         garbage, far, orders, failed);
  return failed ? 1 : 0;
}
