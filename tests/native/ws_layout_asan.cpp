// Every workspace description of csrc/ws_layout.h under AddressSanitizer + UBSan, host code only (no HIP
// call is made; nothing of the library is linked). For each description and size: measure it over null,
// malloc exactly that many bytes, carve, write every array end to end (ASan sees a write past the
// buffer), and check that each array is aligned to its type, that the arrays are pairwise disjoint and
// inside the buffer, and that the area ends on a multiple of 256. A description that a later pipeline
// adds belongs in main() below. Prints the number of layouts walked and of failed checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ws_layout.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

static long g_layouts = 0, g_bad = 0;

static void fail(const char* name, size_t a, size_t b, const char* what) {
  ++g_bad;
  fprintf(stderr, "%s(%zu, %zu): %s\n", name, a, b, what);
}

// describe(Carver&) runs one description; want: the bytes its *_bytes helper (or a formula kept
// elsewhere) gives, which the measured size must equal.
template <class F>
static void walk(const char* name, size_t a, size_t b, size_t want, F describe) {
  ++g_layouts;
  Carver measure(nullptr);
  describe(measure);
  const size_t bytes = measure.bytes();
  if (bytes != want) fail(name, a, b, "measured size differs from its bytes helper");
  if (bytes % 256) fail(name, a, b, "the area does not end on a multiple of 256");
  unsigned char* buf = static_cast<unsigned char*>(malloc(bytes ? bytes : 1));
  if (!buf) exit(2);
  std::vector<Take> takes;
  Carver carve(buf, &takes);
  describe(carve);
  if (carve.bytes() != bytes) fail(name, a, b, "carving and measuring disagree");
  size_t end = 0;  // takes come in order: disjoint when none starts before the one ahead of it ends
  for (const Take& t : takes) {
    if (t.off % t.align) fail(name, a, b, "an array is not aligned to its type");
    if (t.off < end) fail(name, a, b, "two arrays overlap");
    if (t.off + t.bytes > bytes) fail(name, a, b, "an array leaves the buffer");
    if (t.off + t.bytes <= bytes) memset(buf + t.off, 0xA5, t.bytes);
    end = t.off + t.bytes;
  }
  for (size_t i = 0; i < takes.size(); ++i)  // pairwise, whatever the order
    for (size_t j = i + 1; j < takes.size(); ++j)
      if (takes[i].off < takes[j].off + takes[j].bytes && takes[j].off < takes[i].off + takes[i].bytes &&
          takes[i].bytes && takes[j].bytes)
        fail(name, a, b, "two arrays overlap (pairwise)");
  free(buf);
}

int main() {
  const size_t ms[] = {1, 2, 409, 410, 512, 513, 1024, 1025, 2048, 2049, 65536};
  const uint64_t region_lens[] = {0, 1, 4096, (1u << 20) + 1};
  for (size_t m : ms) {
    for (size_t n : {m, (size_t)kMsgSlots * m})
      walk("plan_scratch", n, 0, ws_need(n), [&](Carver& c) {
        PlanArgs p;
        plan_scratch(c, n, p);
      });
    for (int own_out = 0; own_out < 2; ++own_out)
      walk("verify_scratch", m, own_out, ws_need(m) + (own_out ? (m * 4 + 255) / 256 * 256 : 0),
           [&](Carver& c) { verify_scratch(c, m, own_out != 0); });
    walk("msg_jobs", m, 0, msg_jobs_bytes(m), [&](Carver& c) {
      MsgArgs a;
      msg_jobs(c, m, a);
    });
    walk("long_list", m, 0, msg_jobs_bytes(m), [&](Carver& c) {  // fills the job arrays' space, never more
      LongList l;
      long_list(c, msg_jobs_bytes(m), l);
      c.align(256);
    });
    for (uint64_t len : region_lens)
      for (uintptr_t addr : {uintptr_t(4096), uintptr_t(4096 + 63)}) {  // the address is only looked at
        const uint8_t* region = reinterpret_cast<const uint8_t*>(addr);
        walk("region_sums", m, (size_t)len, region_ws_bytes(region, len, m), [&](Carver& c) {
          FusedArgs f;
          region_sums(c, region, len, m, f);
        });
      }
    walk("put_core", m, 0, put_core_bytes(m), [&](Carver& c) {
      PutArgs a;
      put_core(c, m, a);
    });
    walk("transform_own", m, 0, transform_own_bytes(m), [&](Carver& c) {
      TransformArgs t;
      transform_own(c, m, t);
    });
    walk("hd_own", m, 0, hd_own_bytes(m), [&](Carver& c) {
      HdArgs a;
      hd_own(c, m, a);
    });
    walk("rekey_own", m, 0, rekey_own_bytes(m), [&](Carver& c) {
      RekeyArgs a;
      rekey_own(c, m, a);
    });
    walk("send_own", m, 0, send_own_bytes(m), [&](Carver& c) {
      SendArgs a;
      send_own(c, m, a);
    });
    walk("trailed_own", m, 0, trailed_own_bytes(m), [&](Carver& c) {
      TrailerArgs a;
      trailed_own(c, m, a);
    });
    for (uint64_t len : region_lens)
      walk("chain_ws", (size_t)len, m, chain_bytes(len, m), [&](Carver& c) {
        ChainArgs a;
        chain_ws(c, len, m, a);
      });
  }
  printf("layouts=%ld bad=%ld\n", g_layouts, g_bad);
  return g_bad ? 1 : 0;
}
