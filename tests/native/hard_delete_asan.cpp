// ambrycrc_hard_delete_message_cpu under AddressSanitizer + UBSan: it parses untrusted log bytes and
// writes in place, so each message of the region (written by tests/test_hard_delete_cpu.py) is run on an
// exactly-sized copy, on every tail truncation of it, with bytes of its header and of its user-metadata
// and blob record heads flipped, and with random recovery structs. After every call the bytes outside
// [start, start + size) of a deleted message, and every byte of a refused or plan_only one, must be as
// before. Host code only (no HIP call is made). Prints the number of runs and of violations.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ambrycrc.h"
#include "harness_io.h"

static long runs = 0, bad = 0;

static void run(const unsigned char* msg, size_t n, const ambrycrc_hard_delete_info* rec) {
  unsigned char* r = (unsigned char*)malloc(n ? n : 1);  // exactly sized: one byte past it is a report
  if (n) memcpy(r, msg, n);
  uint32_t st = 0, st2 = 0;
  ambrycrc_hard_delete_info plan, info;
  (void)ambrycrc_hard_delete_message_cpu(r, n, 0, rec, 1, &st, &plan);
  if (n && memcmp(r, msg, n) != 0) ++bad;  // plan_only writes nothing
  (void)ambrycrc_hard_delete_message_cpu(r, n, 0, rec, 0, &st2, &info);
  if (st != st2 || memcmp(&plan, &info, sizeof info) != 0) ++bad;
  uint64_t lo = 0, hi = 0;  // the bytes the call may have changed
  if (st2 == 0) {
    lo = info.start;
    hi = lo + info.size;
    if (hi > n || hi < lo) {
      ++bad;
      lo = hi = 0;
    }
  }
  if ((lo && memcmp(r, msg, lo) != 0) || (hi < n && memcmp(r + hi, msg + hi, n - hi) != 0)) ++bad;
  free(r);
  ++runs;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::vector<unsigned char> all = slurp(argv[1]);
  std::vector<uint64_t> offs(4096);
  const size_t m = ambrycrc_chain_messages_host(all.data(), all.size(), 0, offs.data(), offs.size());
  for (size_t i = 0; i < m; ++i) {
    const size_t lo = offs[i], hi = i + 1 < m ? offs[i + 1] : all.size();
    std::vector<unsigned char> msg(all.begin() + lo, all.begin() + hi);
    run(msg.data(), msg.size(), nullptr);
    uint32_t st = 0;
    ambrycrc_hard_delete_info good;
    {
      std::vector<unsigned char> c(msg);
      (void)ambrycrc_hard_delete_message_cpu(c.data(), c.size(), 0, nullptr, 1, &st, &good);
    }
    // every tail truncation: size - 1 is where an off-by-one in the bounds would write past the end
    for (size_t cut = 0; cut < msg.size(); ++cut) {
      run(msg.data(), cut, nullptr);
      if (st == 0) run(msg.data(), cut, &good);
    }
    // flips in the header (the first 64 bytes) and, for a PUT, in the two record heads
    const size_t um = st == 0 ? good.start : 0, bl = st == 0 ? um + 14 + good.usermeta_size : 0;
    for (int t = 0; t < 300; ++t) {
      std::vector<unsigned char> x(msg);
      for (int k = 0; k < 3; ++k) {
        const uint64_t v = lcg_next();
        const size_t base = st != 0 || t < 100 ? 0 : t < 200 ? um : bl;
        const size_t span = base == 0 ? 64 : 24;
        const size_t at = base + (size_t)(v >> 8) % span;
        if (at < x.size()) x[at] ^= (unsigned char)(1u << (v & 7));
      }
      run(x.data(), x.size(), nullptr);
      if (st == 0) run(x.data(), x.size(), &good);
    }
    // recovery structs: the message's own with fields nudged or replaced, then random ones
    for (int t = 0; t < 300; ++t) {
      ambrycrc_hard_delete_info r = good;
      if (st != 0 || t >= 200) {
        unsigned char* p = (unsigned char*)&r;
        for (size_t k = 0; k < sizeof r; ++k) p[k] = (unsigned char)lcg_next();
        if (t & 1) r.header_version = 3, r.usermeta_version = 1, r.blob_version = (int16_t)(1 + lcg_next() % 3), r.blob_type = 0;
      } else {
        switch (lcg_next() % 6) {
          case 0: r.usermeta_size += (uint32_t)(lcg_next() % 5) - 2; break;
          case 1: r.blob_size += lcg_next() % 5 - 2; break;
          case 2: r.blob_size = lcg_next() << (lcg_next() % 40); break;
          case 3: r.blob_version = (int16_t)(lcg_next() % 6); break;
          case 4: r.blob_type = (int16_t)(lcg_next() % 4 - 1); break;
          default: r.usermeta_size = (uint32_t)lcg_next(); break;
        }
      }
      run(msg.data(), msg.size(), &r);
    }
  }
  printf("runs=%ld messages=%zu bad=%ld\n", runs, m, bad);
  return m && bad == 0 ? 0 : 1;
}
