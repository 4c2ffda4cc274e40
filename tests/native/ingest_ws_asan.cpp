// The ingest workspace of csrc/ws_layout.h (ingest_own, then the shared area: the batch's scratch for the
// kIngestSegs jobs a request, which the placement scan and the copy scan reuse) under AddressSanitizer +
// UBSan, host code only. For each size: measure over null, malloc exactly that many bytes, carve, write
// every array end to end, and check that each array is aligned to its type, that the arrays are disjoint
// and inside the buffer, that the area ends on a multiple of 256 and that the two smaller scans fit the
// shared area. Prints the number of layouts walked and of failed checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ws_layout.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

static long g_layouts = 0, g_bad = 0;

static void fail(size_t m, const char* what) {
  ++g_bad;
  fprintf(stderr, "ingest(%zu): %s\n", m, what);
}

template <class F>
static void walk(size_t m, size_t want, F describe) {
  ++g_layouts;
  Carver measure(nullptr);
  describe(measure);
  const size_t bytes = measure.bytes();
  if (bytes != want) fail(m, "measured size differs from its bytes helper");
  if (bytes % 256) fail(m, "the area does not end on a multiple of 256");
  unsigned char* buf = static_cast<unsigned char*>(malloc(bytes ? bytes : 1));
  if (!buf) exit(2);
  std::vector<Take> takes;
  Carver carve(buf, &takes);
  describe(carve);
  if (carve.bytes() != bytes) fail(m, "carving and measuring disagree");
  size_t end = 0;
  for (const Take& t : takes) {
    if (t.off % t.align) fail(m, "an array is not aligned to its type");
    if (t.off < end) fail(m, "two arrays overlap");
    if (t.off + t.bytes > bytes) fail(m, "an array leaves the buffer");
    if (t.off + t.bytes <= bytes) memset(buf + t.off, 0xA5, t.bytes);
    end = t.off + t.bytes;
  }
  free(buf);
}

int main() {
  const size_t ms[] = {1, 2, 409, 410, 512, 513, 1024, 1025, 2048, 2049, 65536};
  for (size_t m : ms) {
    walk(m, ingest_own_bytes(m), [&](Carver& c) {
      IngestArgs a;
      ingest_own(c, m, a);
    });
    // the whole workspace as the entry carves it: the own area, then each user of the shared area in turn
    const size_t shared = ws_need((size_t)kIngestSegs * m);
    for (size_t n : {(size_t)kIngestSegs * m, m, (size_t)kIngestSlots * m}) {
      if (ws_need(n) > shared) fail(m, "a scan does not fit the shared area");
      walk(m, ingest_own_bytes(m) + ws_need(n), [&](Carver& c) {
        IngestArgs a;
        ingest_own(c, m, a);
        PlanArgs p;
        plan_scratch(c, n, p);
      });
    }
  }
  printf("layouts=%ld bad=%ld\n", g_layouts, g_bad);
  return g_bad ? 1 : 0;
}
