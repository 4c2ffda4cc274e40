// The PutRequest wire parse of csrc/put_request.h under AddressSanitizer + UBSan, host code only (nothing of
// the library is linked; the CRC here is the bitwise loop). Every frame sits in a malloc of exactly its
// length, so a read past the wire buffer is seen. For a clean frame of each request version: every
// truncation length, once with the size field left alone (the frame leaves the buffer) and once with the
// size field set to the truncated length (the fields leave the frame); then seeded mutations of single
// bytes and of the size, length and reference fields. After a parse that accepts: the segments must lie
// inside the frame, and the verdict, the properties re-encoding and the MessageInfo are run over it.
// Prints the number of frames parsed and of failed checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crc32_gf2.h"
#include "put_request.h"

using namespace ambrycrc;

static long g_frames = 0, g_bad = 0;

static uint32_t crc_bits(uint32_t crc, const uint8_t* p, size_t n) {
  uint32_t c = ~crc;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

static void be(std::vector<uint8_t>& v, uint64_t x, int n) {
  for (int i = n - 1; i >= 0; --i) v.push_back((uint8_t)(x >> (8 * i)));
}
static void fill(std::vector<uint8_t>& v, size_t n, uint8_t seed) {
  for (size_t i = 0; i < n; ++i) v.push_back((uint8_t)(seed + 31 * i) | 1);
}

static std::vector<uint8_t> clean_frame(int version, int serde, uint32_t key_len, uint32_t enc_len) {
  std::vector<uint8_t> b;  // the CRC'd span
  fill(b, key_len, 3);
  be(b, (uint64_t)serde, 2);
  be(b, 3600, 8);
  b.push_back(2);  // a non-canonical `private`
  be(b, 1700000000000ull, 8);
  be(b, 50, 8);
  for (int s = 0; s < 3; ++s) {
    be(b, 5, 4);
    for (int i = 0; i < 5; ++i) b.push_back((uint8_t)('a' + i));
  }
  if (serde > 1) be(b, 0x00650005, 4);
  if (serde > 2) b.push_back(1);
  if (serde > 3) be(b, 0, 4), be(b, 0, 4);
  if (serde > 4) be(b, 0, 4);
  be(b, 33, 4);
  fill(b, 33, 9);
  be(b, 1, 2);
  if (version >= 4) be(b, enc_len, 2), fill(b, enc_len, 17);
  if (version >= 5) b.push_back(1);
  be(b, 50, 8);
  fill(b, 50, 29);
  std::vector<uint8_t> f;
  be(f, 8 + 2 + 2 + 4 + 4 + 6 + b.size() + 8, 8);
  be(f, 0, 2);
  be(f, (uint64_t)version, 2);
  be(f, 77, 4);
  be(f, 6, 4);
  fill(f, 6, 41);
  f.insert(f.end(), b.begin(), b.end());
  be(f, crc_bits(0, b.data(), b.size()), 8);
  return f;
}

// Parse the n bytes at src, copied into a malloc of exactly n; returns the status, *accepted = the plan.
static uint32_t parse_exact(const uint8_t* src, size_t n, ambrycrc_put_request_ref r, bool expect_clean) {
  uint8_t* wire = static_cast<uint8_t*>(malloc(n ? n : 1));
  if (!wire) exit(2);
  memcpy(wire, src, n);
  ++g_frames;
  const auto crc = [](const uint8_t* b, uint32_t k) { return crc_bits(0, b, k); };
  IngestPlan p;
  const uint32_t st = ingest_parse(wire, n, r, crc, &p);
  if (st == 0) {
    uint64_t off[kIngestSegs], len[kIngestSegs];
    ingest_segments(p, off, len);
    for (uint32_t k = 0; k < kIngestSegs; ++k)
      if (off[k] > n || len[k] > n - off[k]) ++g_bad, fprintf(stderr, "segment %u leaves the buffer\n", k);
    if (ingest_crc_off(p) + 8 > n) ++g_bad, fprintf(stderr, "the CRC leaves the buffer\n");
    const uint32_t whole = crc_bits(0, wire + p.body, ingest_crc_off(p) - p.body);
    uint32_t seg[kIngestSegs];
    for (uint32_t k = 0; k < kIngestSegs; ++k) seg[k] = crc_bits(0, wire + off[k], len[k]);
    const uint32_t comb = ingest_wire_crc(p, seg, [](uint32_t v, uint64_t k) { return gf2_mul(v, xpow8(k)); });
    if (comb != whole) ++g_bad, fprintf(stderr, "combined CRC %08x, whole span %08x\n", comb, whole);
    for (int hv = 1; hv <= 3; ++hv) {
      ambrycrc_put_desc d;
      const uint32_t vs = ingest_verdict(wire, p, whole, hv, &d);
      PutLayout L;
      if (vs == 0 && put_layout(d, L)) {
        ambrycrc_message_info info;
        ingest_info(wire, p, d, L, 0, &info);
        const PropsFix x = ingest_props_fix(p);
        uint32_t acc = 0;
        for (uint32_t j = 0; j < d.props_len; ++j)
          acc += props_v5_byte(x, j, j < x.stored_len ? wire[d.props_src + j] : 0);
        if (info.size != L.length || acc == 0) ++g_bad, fprintf(stderr, "info / properties\n");
      } else if (expect_clean) {
        ++g_bad, fprintf(stderr, "a clean frame got verdict %x\n", vs);
      }
    }
  } else if (expect_clean) {
    ++g_bad, fprintf(stderr, "a clean frame was refused: %x\n", st);
  }
  free(wire);
  return st;
}

int main() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  const auto next = [&]() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
  };
  for (int version = 3; version <= 5; ++version)
    for (int serde = 1; serde <= 5; ++serde)
      for (uint32_t enc_len : {0u, 20u}) {
        const uint32_t key_len = 24;
        const std::vector<uint8_t> f = clean_frame(version, serde, key_len, enc_len);
        const ambrycrc_put_request_ref r{0, key_len, 0};
        parse_exact(f.data(), f.size(), r, true);
        for (size_t n = 0; n < f.size(); ++n) {
          if (parse_exact(f.data(), n, r, false) == 0) ++g_bad, fprintf(stderr, "a cut frame was accepted (%zu)\n", n);
          if (n >= 8) {  // the size field says n
            std::vector<uint8_t> g(f.begin(), f.begin() + n);
            for (int i = 0; i < 8; ++i) g[i] = (uint8_t)((uint64_t)n >> (8 * (7 - i)));
            if (parse_exact(g.data(), n, r, false) == 0) ++g_bad, fprintf(stderr, "a short frame was accepted (%zu)\n", n);
          }
        }
        for (int k = 0; k < 400; ++k) {  // mutations: any status, no read outside the malloc
          std::vector<uint8_t> g = f;
          ambrycrc_put_request_ref q = r;
          const uint64_t what = next() % 6;
          if (what == 0) g[next() % g.size()] ^= (uint8_t)(1u << (next() % 8));
          else if (what == 1) g[next() % g.size()] = (uint8_t)next();
          else if (what == 2) for (int i = 0; i < 8; ++i) g[i] = (uint8_t)next();
          else if (what == 3) q.key_len = (uint32_t)(next() % (2 * g.size()));
          else if (what == 4) q.off = next() % (g.size() + 4);
          else {  // a 4-B field somewhere set to an extreme
            const size_t at = next() % (g.size() - 4);
            const uint32_t v = (next() & 1) ? 0xFFFFFFFFu : 0x7FFFFFFFu;
            for (int i = 0; i < 4; ++i) g[at + i] = (uint8_t)(v >> (8 * (3 - i)));
          }
          parse_exact(g.data(), g.size(), q, false);
        }
      }
  printf("frames=%ld bad=%ld\n", g_frames, g_bad);
  return g_bad ? 1 : 0;
}
