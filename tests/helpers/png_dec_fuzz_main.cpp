// Stand-alone damage run of csrc/png_dec_core.h (through the serial driver of png_dec_host.cpp), built with
// -fsanitize=address,undefined by tests/test_png_dec_core_host.py and run as a subprocess: a 9x7 RGB file and a 70x3 grey file, each
// cut at every length, with every single bit of the first 400 bytes flipped, and with 2000 seeded random byte edits.  Every case must
// end as a non-zero status or as the right pixels; the sanitizer judges the reads and writes.  The files are exact-size heap copies,
// so one byte read past a file is an error.  Half of the flips and edits have the IDAT's CRC mended afterwards, so that the damage
// reaches the layers behind it; such a file can be a VALID other file (a few damaged streams keep their Adler-32): when it decodes
// to other pixels it is written to the directory argv[1] as alt_<k>.png / alt_<k>.raw, and the test asks Pillow whether those are
// the file's pixels.  Prints one summary line; exit code 0 = all cases held.
#include <stdio.h>
#include "png_host.cpp"
#include "png_dec_host.cpp"

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static long cases = 0, declined = 0, decoded = 0, alt = 0;
static const char* alt_dir = nullptr;

static bool run(const std::vector<uint8_t>& file, const std::vector<uint8_t>& pixels, bool must_decline, bool mended = false) {
  uint8_t* f = (uint8_t*)malloc(file.size() ? file.size() : 1);           // exact size: the sanitizer sees any read past the end
  if (!file.empty()) memcpy(f, file.data(), file.size());
  uint8_t* out = (uint8_t*)malloc(pixels.size());
  memset(out, 0xA5, pixels.size());
  int32_t info[PNGD_INFO_WORDS], stats[4];
  const int st = png_dec_host_decode(f, (int64_t)file.size(), 16, 4, 3, 0, out, (int64_t)pixels.size(), info, stats);
  bool ok = true;
  ++cases;
  if (st == 0) {
    const bool same = memcmp(out, pixels.data(), pixels.size()) == 0;
    if (same) ++decoded;
    ok = !must_decline && (same || (mended && alt_dir));
    if (ok && !same) {
      char name[512];
      for (int part = 0; part < 2; ++part) {
        snprintf(name, sizeof name, "%s/alt_%ld.%s", alt_dir, alt, part ? "raw" : "png");
        FILE* fo = fopen(name, "wb");
        if (!fo) { ok = false; break; }
        if (part) fwrite(out, 1, pixels.size(), fo); else fwrite(file.data(), 1, file.size(), fo);
        fclose(fo);
      }
      ++alt;
    }
  } else {
    ++declined;
    for (size_t k = 0; k < pixels.size(); ++k) ok = ok && out[k] == 0xA5;   // nothing written before the decision
  }
  free(f); free(out);
  return ok;
}

static void mend_idat_crc(std::vector<uint8_t>& g) {
  const size_t n = g.size();
  const uint32_t c = pngd_host_crc(g.data() + 37, n - 16 - 37);
  g[n - 16] = (uint8_t)(c >> 24); g[n - 15] = (uint8_t)(c >> 16); g[n - 14] = (uint8_t)(c >> 8); g[n - 13] = (uint8_t)c;
}

static int damage(int H, int W, int C) {
  std::vector<uint8_t> pix((size_t)H * W * C);
  for (size_t k = 0; k < pix.size(); ++k) pix[k] = (uint8_t)((k * 37 + (k / 5) * 11 + (rnd() & 7)) & 0xff);
  std::vector<uint8_t> file(4096 + 4 * pix.size());
  const int64_t n = png_host_encode(pix.data(), H, W, C, file.data(), (int64_t)file.size(), 256);
  if (n <= 0) return 1;
  file.resize((size_t)n);
  const long before = decoded;
  if (!run(file, pix, false) || decoded != before + 1) { printf("the undamaged %dx%dx%d file does not decode\n", H, W, C); return 1; }
  for (size_t cut = 0; cut < file.size(); ++cut) {
    std::vector<uint8_t> g(file.begin(), file.begin() + cut);
    if (!run(g, pix, true)) { printf("truncation to %zu bytes: wrong result\n", cut); return 1; }
  }
  // the file is signature, IHDR, ONE IDAT, IEND: the IDAT's type starts at byte 37, its CRC 16 bytes before the end.  With the CRC
  // mended after the damage (fix = 1) the damage reaches the zlib header, the code table, the Huffman data and the Adler-32.
  const size_t nb = file.size() < 400 ? file.size() : 400;
  for (int fix = 0; fix < 2; ++fix) {
    for (size_t bit = 0; bit < nb * 8; ++bit) {
      std::vector<uint8_t> g(file);
      g[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
      if (fix) mend_idat_crc(g);
      if (!run(g, pix, false, fix)) { printf("bit flip %zu (crc mended: %d): wrong result\n", bit, fix); return 1; }
    }
    for (int k = 0; k < 2000; ++k) {
      std::vector<uint8_t> g(file);
      const int edits = 1 + (int)(rnd() % 3);
      for (int e = 0; e < edits; ++e) g[rnd() % g.size()] = (uint8_t)rnd();
      if (fix) mend_idat_crc(g);
      if (!run(g, pix, false, fix)) { printf("random edit %d (crc mended: %d): wrong result\n", k, fix); return 1; }
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) alt_dir = argv[1];
  if (damage(7, 9, 3)) return 1;
  if (damage(3, 70, 1)) return 1;
  printf("png_dec_fuzz: %ld cases, %ld declined, %ld decoded to the right pixels, %ld valid other files\n", cases, declined, decoded, alt);
  return 0;
}
