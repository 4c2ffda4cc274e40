// The GET receive of csrc/recv.h under AddressSanitizer + UBSan, host code only (nothing of the library is
// linked; the CRC here is the bitwise loop): recv_plan and the whole CPU entry (recv_blob_host, which
// ambrycrc_receive_blob_cpu only wraps). argv[1] is a file of payloads, each [u32 flag][u32 length][bytes],
// little-endian, all clean. Every payload sits in a malloc of exactly its length, so a read past `avail` is
// seen. For each payload: the clean run (status 0, the delivered bytes the content's), every truncation
// length (never clean: a cut record or message is refused), one flipped bit in turn in every byte of the
// first 96 and the last 24 bytes and in sampled bytes between, each under several ranges and output
// capacities. Whatever the status, a delivered span must lie inside the payload and the output buffer, which
// is exactly out_cap bytes. Then the struct's size and field offsets are printed, and the receive workspace
// (ws_layout.h recv_own, then the verify's job arrays and the batch scratch) is carved over exactly its
// measured size and written end to end. Prints the number of runs, of layouts and of failed checks.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "recv.h"
#include "ws_layout.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

static long g_runs = 0, g_layouts = 0, g_bad = 0;

static uint32_t crc_bits(const uint8_t* p, uint64_t n) {
  uint32_t c = ~0u;
  for (uint64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

static void fail(const char* what, size_t n) {
  ++g_bad;
  fprintf(stderr, "%s (%zu)\n", what, n);
}

// One receive of the n bytes at src, copied into a malloc of exactly n, into an output of exactly cap bytes.
static uint32_t run(const uint8_t* src, size_t n, int flag, uint64_t lo, uint64_t hi, uint64_t cap,
                    ambrycrc_recv_info* info_out = nullptr, std::vector<uint8_t>* bytes = nullptr) {
  uint8_t* p = static_cast<uint8_t*>(malloc(n ? n : 1));
  uint8_t* out = static_cast<uint8_t*>(malloc(cap ? cap : 1));
  if (!p || !out) exit(2);
  memcpy(p, src, n);
  ++g_runs;
  ambrycrc_recv_info info;
  uint32_t st = ~0u;
  recv_blob_host(p, n, flag, lo, hi, cap ? out : nullptr, cap, crc_bits, &info, &st);
  const uint32_t crc_only = AMBRYCRC_MSG_ENCKEY_CRC | AMBRYCRC_MSG_PROPS_CRC | AMBRYCRC_MSG_USERMETA_CRC | AMBRYCRC_MSG_BLOB_CRC;
  if (st & ~crc_only) {
    if (info.out_off != kRecvNowhere || info.out_len || info.blob_size || info.content_rel || info.blob_version)
      fail("a refused payload reports info", n);
  } else {
    if (info.out_off != 0) fail("a delivered payload is nowhere", n);
    if (info.out_len > cap) fail("the slice leaves the output", n);
    if ((uint64_t)info.content_rel + info.blob_size + 8 > n) fail("the record leaves the payload", n);
    if (info.out_len > info.blob_size) fail("the slice is longer than the content", n);
    if (st == 0 && info.out_len && memcmp(out, p + info.content_rel + lo, info.out_len)) fail("delivered bytes differ", n);
    if ((uint64_t)info.enckey_rel + info.enckey_len > n || (uint64_t)info.props_rel + info.props_len > n ||
        (uint64_t)info.usermeta_rel + info.usermeta_len > n)
      fail("a field leaves the payload", n);
  }
  if (info_out) *info_out = info;
  if (bytes) bytes->assign(out, out + (st & ~crc_only ? 0 : info.out_len));
  free(p);
  free(out);
  return st;
}

static void payload(const std::vector<uint8_t>& b, int flag) {
  const size_t n = b.size();
  ambrycrc_recv_info info;
  if (run(b.data(), n, flag, 0, kRecvToEnd, n, &info) != 0) return fail("a clean payload was not delivered", n);
  const uint64_t size = info.blob_size;
  const uint64_t ranges[][2] = {{0, kRecvToEnd}, {0, 0}, {size / 3, size - size / 4}, {size, size}, {1, size + 1}, {5, 4}};
  for (const auto& r : ranges) {
    const uint32_t st = run(b.data(), n, flag, r[0], r[1], n);
    const bool valid = r[0] <= (r[1] == kRecvToEnd ? size : r[1]) && (r[1] == kRecvToEnd || r[1] <= size);
    if (st != (valid ? 0u : (uint32_t)AMBRYCRC_MSG_BAD_RANGE)) fail("a range's status", (size_t)r[0]);
  }
  if (size && run(b.data(), n, flag, 0, kRecvToEnd, size - 1) != AMBRYCRC_MSG_NO_ROOM) fail("one byte short of room", n);
  if (run(b.data(), n, flag, 0, kRecvToEnd, size) != 0) fail("exactly enough room", n);
  // truncations: with trailing bytes cut away a payload may still be whole; below its own end it never is
  const uint64_t own_end = (uint64_t)info.content_rel + size + 8;
  for (size_t cut = 0; cut < n; ++cut) {
    if (n > 4096 && cut > 200 && cut + 200 < n && cut % 97) continue;
    const uint32_t st = run(b.data(), cut, flag, 0, kRecvToEnd, n);
    if (st == 0 && cut < own_end) fail("a cut payload was delivered", cut);
  }
  uint64_t rng = 0x9E3779B97F4A7C15ull ^ n;
  std::vector<uint8_t> g = b;
  for (size_t at = 0; at < n; ++at) {
    if (at >= 96 && at + 24 < n && at % 61) continue;
    for (int bit = 0; bit < 8; ++bit) {
      rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
      g[at] ^= (uint8_t)(1u << bit);
      run(g.data(), n, flag, 0, kRecvToEnd, n);
      run(g.data(), n, flag, rng % (size + 1), rng % (size + 2) ? kRecvToEnd : size, (size_t)(rng >> 20) % (n + 1));
      g[at] ^= (uint8_t)(1u << bit);
    }
  }
}

static void layouts() {
  const size_t ms[] = {1, 2, 409, 410, 2048, 2049, 65536};
  for (size_t m : ms) {
    for (size_t slots : {(size_t)kRecvSlotsBlob, (size_t)kRecvSlotsAll}) {
      ++g_layouts;
      const bool all = slots == kRecvSlotsAll;
      // as ambrycrc_recv.cpp carves it: the own area, (ALL) the verify's job arrays, then each user of the
      // batch area in turn -- the placement scan of m lengths, the CRC pass over slots * m jobs
      for (size_t n : {m, slots * m}) {
        const auto describe = [&](Carver& c) {
          RecvArgs a;
          recv_own(c, m, a);
          if (all) {
            MsgArgs ma;
            msg_jobs(c, m, ma);
          }
          PlanArgs p;
          plan_scratch(c, n, p);
        };
        Carver measure(nullptr);
        describe(measure);
        const size_t bytes = measure.bytes();
        if (bytes > recv_ws_bytes(m)) fail("a carving needs more than the workspace size", m);
        if (all && n == slots * m && bytes != recv_ws_bytes(m)) fail("the workspace size is not the largest carving", m);
        unsigned char* buf = static_cast<unsigned char*>(malloc(bytes));
        if (!buf) exit(2);
        std::vector<Take> takes;
        Carver carve(buf, &takes);
        describe(carve);
        size_t end = 0;
        for (const Take& t : takes) {
          if (t.off % t.align) fail("an array is not aligned to its type", m);
          if (t.off < end) fail("two arrays overlap", m);
          if (t.off + t.bytes > bytes) fail("an array leaves the buffer", m);
          else memset(buf + t.off, 0xA5, t.bytes);
          end = t.off + t.bytes;
        }
        free(buf);
      }
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  for (;;) {
    uint32_t h[2];
    if (fread(h, 4, 2, f) != 2) break;
    std::vector<uint8_t> b(h[1]);
    if (h[1] && fread(b.data(), 1, h[1], f) != h[1]) return 2;
    payload(b, (int)h[0]);
  }
  fclose(f);
  layouts();
  printf("sizeof=%zu", sizeof(ambrycrc_recv_info));
#define FIELD(name) printf(" %s=%zu", #name, offsetof(ambrycrc_recv_info, name))
  FIELD(out_off), FIELD(out_len), FIELD(blob_size), FIELD(content_rel), FIELD(enckey_rel), FIELD(enckey_len);
  FIELD(props_rel), FIELD(props_len), FIELD(usermeta_rel), FIELD(usermeta_len), FIELD(blob_type), FIELD(compressed);
  FIELD(blob_version), FIELD(header_version);
  printf("\nruns=%ld layouts=%ld bad=%ld\n", g_runs, g_layouts, g_bad);
  return g_bad ? 1 : 0;
}
