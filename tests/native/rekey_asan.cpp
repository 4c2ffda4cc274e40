// ambrycrc_rekey_message_cpu under AddressSanitizer + UBSan: it parses untrusted log bytes and follows
// untrusted descriptor offsets into aux. Each message of the region (written by tests/test_rekey_cpu.py,
// 30 % of them corrupted) is run as an exactly-sized heap copy, with an exactly-sized aux and output, at
// every header version; on every tail truncation of the message; with its descriptor's spans moved to
// both ends of aux and one byte past them, aux cut short under a descriptor, and random descriptors.
// A span outside aux must be AMBRYCRC_MSG_BAD_DESC; an output must fit exactly its reported length and
// be refused one byte short. Host code only (no HIP call is made). Prints the runs and the violations.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ambrycrc.h"
#include "harness_io.h"

static long runs = 0, bad = 0, written = 0;

static bool spans_ok(const ambrycrc_rekey_desc& d, uint64_t aux_len) {
  if (d.key_src > aux_len || d.key_len > aux_len - d.key_src) return false;
  if (d.content_src == UINT64_MAX) return true;
  return d.content_len <= 0x7FFFFFFFull && d.content_src <= aux_len && d.content_len <= aux_len - d.content_src;
}

// One call on exactly-sized copies: one byte read or written past any of them is a report.
static void run(const unsigned char* msg, size_t n, const ambrycrc_rekey_desc& d, const unsigned char* aux,
                size_t aux_len, int hv) {
  unsigned char* r = (unsigned char*)malloc(n ? n : 1);
  unsigned char* a = (unsigned char*)malloc(aux_len ? aux_len : 1);
  if (n) memcpy(r, msg, n);
  if (aux_len) memcpy(a, aux, aux_len);
  const uint64_t cap = ambrycrc_rekey_out_bound(n, 1, aux_len);
  unsigned char* o = (unsigned char*)malloc(cap ? cap : 1);
  uint32_t st = 0;
  uint64_t len = 0;
  const int rc = ambrycrc_rekey_message_cpu(r, n, 0, &d, aux_len ? a : nullptr, aux_len, (int)(runs % 5) - 1, hv, o, cap,
                                            &len, &st);
  if (rc != AMBRYCRC_OK || len > cap || (st != 0 && len != 0)) ++bad;
  if (st == AMBRYCRC_MSG_NO_ROOM) ++bad;  // the bound holds: one message, its own aux bytes
  if (d.key_len != 0 && !spans_ok(d, aux_len) && st != AMBRYCRC_MSG_BAD_DESC) ++bad;
  if (d.key_len == 0 && (st != 0 || len != 0)) ++bad;
  if (st == 0 && len) {  // exactly its length, and refused one byte short
    ++written;
    unsigned char* e = (unsigned char*)malloc(len);
    uint32_t st2 = 1;
    uint64_t len2 = 0;
    (void)ambrycrc_rekey_message_cpu(r, n, 0, &d, a, aux_len, (int)(runs % 5) - 1, hv, e, len, &len2, &st2);
    if (st2 != 0 || len2 != len || memcmp(e, o, len) != 0) ++bad;
    (void)ambrycrc_rekey_message_cpu(r, n, 0, &d, a, aux_len, -1, hv, e, len - 1, &len2, &st2);
    if (st2 != AMBRYCRC_MSG_NO_ROOM || len2 != 0) ++bad;
    free(e);
  }
  if ((n && memcmp(r, msg, n) != 0) || (aux_len && memcmp(a, aux, aux_len) != 0)) ++bad;  // inputs are read-only
  free(o);
  free(a);
  free(r);
  ++runs;
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::vector<unsigned char> all = slurp(argv[1]), ob = slurp(argv[2]), db = slurp(argv[3]), aux = slurp(argv[4]);
  const size_t m = ob.size() / 8;
  if (!m || db.size() != m * sizeof(ambrycrc_rekey_desc)) return 2;
  std::vector<uint64_t> offs(m);
  std::vector<ambrycrc_rekey_desc> descs(m);
  memcpy(offs.data(), ob.data(), m * 8);
  memcpy(descs.data(), db.data(), db.size());
  const size_t A = aux.size();
  for (size_t i = 0; i < m; ++i) {
    const size_t lo = offs[i], hi = i + 1 < m ? offs[i + 1] : all.size();
    const std::vector<unsigned char> msg(all.begin() + lo, all.begin() + hi);
    const ambrycrc_rekey_desc d0 = descs[i];
    for (int hv = 1; hv <= 3; ++hv) run(msg.data(), msg.size(), d0, aux.data(), A, hv);
    // every tail truncation: size - 1 is where an off-by-one in the bounds would read past the end
    for (size_t cut = 0; cut < msg.size(); ++cut) run(msg.data(), cut, d0, aux.data(), A, 1 + (int)(cut % 3));
    // the descriptor's spans at both ends of aux, and one byte past them
    ambrycrc_rekey_desc d = d0;
    if (d.key_len == 0) d.key_len = 9;
    const uint32_t kl = d.key_len;
    for (int with_content = 0; with_content < 2; ++with_content) {
      const uint64_t cl = 38;
      for (int t = 0; t < 6; ++t) {
        ambrycrc_rekey_desc x = d;
        x.key_src = t == 0 ? 0 : t == 1 ? A - kl : t == 2 ? A - kl + 1 : t == 3 ? A : t == 4 ? UINT64_MAX : A + 1;
        if (with_content) {
          x.content_len = cl;
          x.content_src = t == 0 ? A - cl : t == 1 ? 0 : t == 2 ? 0 : t == 3 ? A - cl + 1 : t == 4 ? A : UINT64_MAX - 1;
        }
        run(msg.data(), msg.size(), x, aux.data(), A, 3);
      }
      ambrycrc_rekey_desc x = d;
      if (with_content) x.content_src = 0, x.content_len = 0x80000000ull;
      run(msg.data(), msg.size(), x, aux.data(), A, 2);
    }
    // aux cut short under the descriptor: the last byte of each span, then one before it
    for (uint64_t end : {d0.key_src + d0.key_len, d0.content_src == UINT64_MAX ? A : d0.content_src + d0.content_len}) {
      for (uint64_t cutA : {end, end - 1}) {
        if (cutA <= A) run(msg.data(), msg.size(), d0, aux.data(), (size_t)cutA, 3);
      }
    }
    run(msg.data(), msg.size(), d0, aux.data(), 0, 3);
    for (int t = 0; t < 200; ++t) {  // random descriptors; every other one with small fields
      ambrycrc_rekey_desc x;
      unsigned char* p = (unsigned char*)&x;
      for (size_t k = 0; k < sizeof x; ++k) p[k] = (unsigned char)lcg_next();
      if (t & 1) {
        x.key_len = (uint32_t)(lcg_next() % 100);
        x.key_src = lcg_next() % (A + 2);
        x.content_len = lcg_next() % 300;
        x.content_src = (t & 2) ? UINT64_MAX : lcg_next() % (A + 2);
      }
      run(msg.data(), msg.size(), x, aux.data(), A, 1 + t % 3);
    }
  }
  printf("runs=%ld messages=%zu written=%ld bad=%ld\n", runs, m, written, bad);
  return m && written && bad == 0 ? 0 : 1;
}
