// What the stand-alone sanitizer harnesses of this folder share: reading an input file whole, and the
// 64-bit LCG (Knuth's MMIX constants, top 40 bits) that draws their mutations. Host code only.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

// The file's bytes; a file that cannot be opened ends the program with status 2.
static inline std::vector<unsigned char> slurp(const char* path) {
  std::vector<unsigned char> all;
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  unsigned char buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) all.insert(all.end(), buf, buf + got);
  fclose(f);
  return all;
}

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static inline uint64_t lcg_next() {
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return lcg_state >> 24;
}
