// ambrycrc_recover_messages_cpu under AddressSanitizer + UBSan: it walks untrusted log bytes, hopping by sizes
// they carry, and reads record fields at offsets they carry. Every region file (written by
// tests/test_recover_cpu.py: the stop cases, a region with 30 % of its messages corrupted, the info edge cases)
// is run as an exactly-sized heap copy, from offset 0 and from every chained message start, with max_m below,
// at and above the chain length, into exactly-sized output arrays, and on tail truncations (the first and last
// 300 cuts and every 89th between). Host code only (no HIP call is made). Prints the runs and the violations.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ambrycrc.h"
#include "harness_io.h"

static long runs = 0, bad = 0, recovered = 0;

// One call on an exactly-sized copy of the first n bytes; the chained starts are appended to *starts.
static ambrycrc_recover_result run(const unsigned char* bytes, size_t n, uint64_t start, size_t max_m,
                                   std::vector<uint64_t>* starts) {
  unsigned char* r = (unsigned char*)malloc(n ? n : 1);
  if (n) memcpy(r, bytes, n);
  uint64_t* off = (uint64_t*)malloc(max_m * sizeof(uint64_t));
  ambrycrc_message_info* info = (ambrycrc_message_info*)malloc(max_m * sizeof(ambrycrc_message_info));
  uint32_t* st = (uint32_t*)malloc(max_m * sizeof(uint32_t));
  ambrycrc_recover_result res;
  memset(&res, 0xEE, sizeof res);
  const int rc = ambrycrc_recover_messages_cpu(r, n, start, max_m, off, info, st, &res);
  ++runs;
  if (rc != AMBRYCRC_OK) {
    ++bad;
  } else {
    if (res.chained > max_m || res.recovered > res.chained || res.end_off > n || res.end_off < start || res.more > 1) ++bad;
    if (res.more && (res.end_status != 0 || res.chained != max_m || res.end_off == n)) ++bad;
    uint64_t prev = start;
    for (size_t i = 0; i < max_m; ++i) {
      const ambrycrc_message_info& f = info[i];
      static const ambrycrc_message_info zero = {};
      if (i >= res.chained) {
        if (off[i] != UINT64_MAX || st[i] != AMBRYCRC_MSG_BAD_LAYOUT || memcmp(&f, &zero, sizeof f) != 0) ++bad;
        continue;
      }
      if (off[i] != prev || off[i] >= n) ++bad;  // each start is where the one before it ends
      if (i < res.recovered ? st[i] != 0 : (i == res.recovered && st[i] == 0)) ++bad;
      if (st[i] != 0) {
        if (memcmp(&f, &zero, sizeof f) != 0) ++bad;
        // the hop does not depend on the records: find the next start from the following slot or the end
        prev = i + 1 < res.chained ? off[i + 1] : prev;
        continue;
      }
      ++recovered;
      if (f.msg_off != off[i] || f.size == 0 || f.size > n - off[i] || f.key_rel < 34 || f.key_rel > 40 ||
          (uint64_t)f.key_rel + f.key_len > f.size || f.header_version < 1 || f.header_version > 3 ||
          f.operation_time_ms < -1 || (f.flags != 0 && f.flags != 1 && f.flags != 2 && f.flags != 4) ||
          (f.flags != 0 && f.expires_at_ms != -1))
        ++bad;
      prev = off[i] + f.size;
    }
    if (res.recovered == res.chained && res.chained && res.end_off != prev && st[res.chained - 1] == 0) ++bad;
    if (starts) starts->insert(starts->end(), off, off + res.chained);
  }
  if (n && memcmp(r, bytes, n) != 0) ++bad;  // the region is read-only
  free(st);
  free(info);
  free(off);
  free(r);
  return res;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int a = 1; a < argc; ++a) {
    const std::vector<unsigned char> all = slurp(argv[a]);
    if (all.empty()) return 2;
    const size_t n = all.size();
    // the whole region, restarting one byte after every stop so that every message is reached
    std::vector<uint64_t> starts;
    for (uint64_t at = 0; at < n;) {
      const ambrycrc_recover_result res = run(all.data(), n, at, 4096, &starts);
      uint64_t next = res.end_off + 1;
      if (res.recovered < res.chained) next = starts.back() + 1;  // past everything this call chained
      at = next > at ? next : at + 1;
      if (runs > 200000) break;
    }
    const size_t m = starts.size() ? starts.size() : 1;
    for (size_t max_m : {(size_t)1, (size_t)2, m - 1 ? m - 1 : 1, m, m + 1}) {
      for (uint64_t at = 0;;) {  // repeated calls while `more` is set
        const ambrycrc_recover_result res = run(all.data(), n, at, max_m, nullptr);
        if (!res.more || res.end_off <= at) break;
        at = res.end_off;
      }
    }
    for (size_t i = 0; i < starts.size(); i += starts.size() > 64 ? 7 : 1) run(all.data(), n, starts[i], 8, nullptr);
    for (size_t cut = 0; cut < n; ++cut)
      if (cut < 300 || cut + 300 >= n || cut % 89 == 0) run(all.data(), cut, 0, 64, nullptr);
    run(all.data(), n, n, 3, nullptr);
    run(all.data(), n, n - 1, 3, nullptr);
    uint64_t off[1];
    ambrycrc_recover_result res;
    if (ambrycrc_recover_messages_cpu(all.data(), n, n + 1, 1, off, nullptr, nullptr, &res) != AMBRYCRC_EINVAL) ++bad;
    if (ambrycrc_recover_messages_cpu(all.data(), n, 0, 0, off, nullptr, nullptr, &res) != AMBRYCRC_EINVAL) ++bad;
    if (ambrycrc_recover_messages_cpu(all.data(), n, 0, 1, nullptr, nullptr, nullptr, &res) != AMBRYCRC_EINVAL) ++bad;
    if (ambrycrc_recover_messages_cpu(all.data(), n, 0, 1, off, nullptr, nullptr, &res) != AMBRYCRC_OK) ++bad;
  }
  printf("runs=%ld recovered=%ld bad=%ld\n", runs, recovered, bad);
  return recovered && bad == 0 ? 0 : 1;
}
