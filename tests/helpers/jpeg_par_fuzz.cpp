// Mutation fuzzer for csrc/jpeg_par_core.h (host build).  Build with -fsanitize=address,undefined: any read or write outside a buffer, on
// any byte soup, aborts.  The mutations are those of jpeg_fuzz.cpp; every mutated file goes through the lane decoder and through the parallel
// route at S = 4, S = 16 and the product geometry, and the two must agree.   usage: jpeg_par_fuzz <iterations> <seed.jpg>...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "jpeg_par_host.cpp"

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize((size_t)n);
  if (fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear();
  fclose(f);
  return v;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const long iters = atol(argv[1]);
  std::vector<std::vector<uint8_t>> seeds;
  for (int i = 2; i < argc; ++i) { auto v = slurp(argv[i]); if (!v.empty()) seeds.push_back(v); }
  if (seeds.empty()) return 2;
  const int64_t cap = (int64_t)3 << 20;
  std::vector<uint8_t> a((size_t)cap), b((size_t)cap);
  long parallel = 0, fell = 0, rejected = 0, mismatches = 0;
  for (long it = 0; it < iters; ++it) {
    std::vector<uint8_t> f = seeds[rnd() % seeds.size()];
    const int kind = rnd() % 6;
    if (kind == 0) {                                   // flip a few bytes anywhere
      for (int k = 0, n = 1 + rnd() % 8; k < n; ++k) f[rnd() % f.size()] = (uint8_t)rnd();
    } else if (kind == 1) {                            // flip bytes in the header region (tables, sizes, sampling factors)
      const size_t hdr = f.size() < 700 ? f.size() : 700;
      for (int k = 0, n = 1 + rnd() % 6; k < n; ++k) f[rnd() % hdr] = (uint8_t)rnd();
    } else if (kind == 2) {                            // truncate
      f.resize(1 + rnd() % f.size());
    } else if (kind == 3) {                            // sprinkle markers / 0xFF bytes into the entropy data
      for (int k = 0, n = 1 + rnd() % 6; k < n; ++k) { const size_t p = f.size() / 2 + rnd() % (f.size() / 2); f[p] = 0xFF; if (p + 1 < f.size() && (rnd() & 1)) f[p + 1] = (uint8_t)(0xC0 + rnd() % 0x40); }
    } else if (kind == 4) {                            // duplicate a slice (repeated segments, shifted offsets)
      const size_t s = rnd() % f.size(), n = rnd() % 300;
      std::vector<uint8_t> g(f.begin(), f.begin() + s);
      g.insert(g.end(), f.begin() + s, f.begin() + (s + n < f.size() ? s + n : f.size()));
      g.insert(g.end(), f.begin() + s, f.end());
      f.swap(g);
    } else {                                           // random bytes behind a valid SOI
      for (size_t k = 2; k < f.size(); ++k) if ((rnd() & 7) == 0) f[k] = (uint8_t)rnd();
    }
    // the file in an exact-size heap block: the helper copies it into its padded blob, so a read past the FILE shows here
    std::vector<uint8_t> file(f);
    int32_t sa[6], sb[6];
    const int st0 = jpeg_par_host_decode(file.data(), (int64_t)file.size(), 0, 0, 0, 0, a.data(), cap, sa);
    if (st0 != 0) { ++rejected; }
    const int geo[3][2] = {{4, 2}, {16, 2}, {JPEG_PAR_S, JPEG_PAR_SPAN}};
    for (int gi = 0; gi < 3; ++gi) {
      const int st1 = jpeg_par_host_decode(file.data(), (int64_t)file.size(), geo[gi][0], geo[gi][1], 1 << 20, 1, b.data(), cap, sb);
      if (st1 != st0) { ++mismatches; continue; }
      if (st0 != 0) continue;
      JpegInfo o;
      jpeg_parse(file.data(), (int64_t)file.size(), &o);
      const size_t px = (size_t)o.width * o.height * 3;
      if (sa[4] != sb[4] || memcmp(a.data(), b.data(), px) != 0) ++mismatches;
      if (gi == 2) { if (sb[0] == 1) ++parallel; else ++fell; }
    }
  }
  printf("iterations %ld: parallel %ld, fell back %ld, rejected %ld, mismatches %ld\n", iters, parallel, fell, rejected, mismatches);
  return mismatches ? 1 : 0;
}
