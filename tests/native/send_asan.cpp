// ambrycrc_send_message_cpu under AddressSanitizer + UBSan: it parses untrusted log bytes and copies spans
// whose bounds come from them. Every message of two regions (written by tests/test_send_cpu.py: the rule
// cases, and a region with 30 % of its messages corrupted) is run as an exactly-sized heap copy under every
// flag, without a size and with sizes around its length, into an output of exactly the bytes it reports,
// and one byte short; then on every tail truncation. A sent span must lie inside the message and equal
// its bytes. Host code only (no HIP call is made). Prints the runs and the violations.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ambrycrc.h"
#include "harness_io.h"

static long runs = 0, bad = 0, sent = 0;

// One call on an exactly-sized copy of the n message bytes: one byte read past it is a report.
static void run(const unsigned char* msg, size_t n, uint64_t size, int flag) {
  unsigned char* r = (unsigned char*)malloc(n ? n : 1);
  if (n) memcpy(r, msg, n);
  unsigned char* o = (unsigned char*)malloc(n ? n : 1);
  ambrycrc_send_info f;
  uint32_t st = 0;
  const int rc = ambrycrc_send_message_cpu(r, n, 0, size, flag, o, n, &f, &st);
  if (rc != AMBRYCRC_OK || st == AMBRYCRC_MSG_NO_ROOM) ++bad;  // a span never exceeds its message
  if (st != 0 && (f.send_len != 0 || f.out_off != UINT64_MAX)) ++bad;
  if (size > n && st != AMBRYCRC_MSG_BAD_LAYOUT) ++bad;
  if (st == 0) {
    ++sent;
    if (f.out_off != 0 || f.send_len == 0 || f.rel_off > n || f.send_len > n - f.rel_off ||
        memcmp(o, r + f.rel_off, f.send_len) != 0)
      ++bad;
    if (f.enckey_rel && ((uint64_t)f.enckey_rel + f.enckey_len > n)) ++bad;
    if (!bad) {  // exactly its length, and refused one byte short
      unsigned char* e = (unsigned char*)malloc(f.send_len);
      ambrycrc_send_info g;
      uint32_t st2 = 1;
      (void)ambrycrc_send_message_cpu(r, n, 0, size, flag, e, f.send_len, &g, &st2);
      if (st2 != 0 || g.send_len != f.send_len || g.check != f.check || memcmp(e, o, f.send_len) != 0) ++bad;
      (void)ambrycrc_send_message_cpu(r, n, 0, size, flag, e, f.send_len - 1, &g, &st2);
      if (st2 != AMBRYCRC_MSG_NO_ROOM || g.send_len != 0 || g.out_off != UINT64_MAX || g.check != f.check) ++bad;
      (void)ambrycrc_send_message_cpu(r, n, 0, size, flag, nullptr, 0, &g, &st2);
      if (st2 != AMBRYCRC_MSG_NO_ROOM) ++bad;
      free(e);
    }
  }
  if (n && memcmp(r, msg, n) != 0) ++bad;  // the region is read-only
  free(o);
  free(r);
  ++runs;
}

static void region_runs(const std::vector<unsigned char>& all, const std::vector<unsigned char>& ob, bool truncate) {
  const size_t m = ob.size() / 8;
  std::vector<uint64_t> offs(m);
  memcpy(offs.data(), ob.data(), m * 8);
  for (size_t i = 0; i < m; ++i) {
    const size_t lo = offs[i], hi = i + 1 < m ? offs[i + 1] : all.size();
    const std::vector<unsigned char> msg(all.begin() + lo, all.begin() + hi);
    const uint64_t n = msg.size();
    for (int flag = 0; flag <= 4; ++flag) {
      for (uint64_t size : {(uint64_t)0, n, n - 1, n - 9, n / 2, (uint64_t)41, (uint64_t)1, n + 1, UINT64_MAX})
        run(msg.data(), n, size, flag);
      // every tail truncation: size - 1 is where an off-by-one in the bounds would read past the end
      // (every flag over the last 128 cuts and the first 128, one flag in turn over the rest)
      if (truncate)
        for (size_t cut = 0; cut < n; ++cut)
          if (cut < 128 || cut + 128 >= n || (int)(cut % 5) == flag) run(msg.data(), cut, (cut & 1) ? cut : 0, flag);
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::vector<unsigned char> all = slurp(argv[1]), ob = slurp(argv[2]), rules = slurp(argv[3]), rb = slurp(argv[4]);
  if (ob.size() < 8 || rb.size() < 8) return 2;
  region_runs(all, ob, true);
  region_runs(rules, rb, false);
  ambrycrc_send_info f;
  uint32_t st = 0;
  if (ambrycrc_send_message_cpu(all.data(), all.size(), 0, 0, 5, nullptr, 0, &f, &st) != AMBRYCRC_EINVAL) ++bad;
  if (ambrycrc_send_message_cpu(all.data(), all.size(), all.size() + 1, 0, 2, nullptr, 0, &f, &st) != AMBRYCRC_OK ||
      st != AMBRYCRC_MSG_BAD_LAYOUT)
    ++bad;
  printf("runs=%ld sent=%ld bad=%ld\n", runs, sent, bad);
  return sent && bad == 0 ? 0 : 1;
}
