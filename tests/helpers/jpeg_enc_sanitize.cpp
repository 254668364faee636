// Stand-alone driver for tests/test_jpeg_enc_core_host.py::test_core_is_clean_under_address_and_ub_sanitizers: the serial composition of
// csrc/jpeg_enc_core.h (jpeg_enc_host.cpp) over random sizes, settings and contents, built with -fsanitize=address,undefined.  On the
// GPU an out-of-bounds access is a memory fault, not an exception: the shared arithmetic has to stay inside its buffers here.
#include <stdio.h>
#include <stdlib.h>

#include "jpeg_enc_host.cpp"

int main(int argc, char** argv) {
  const int iterations = argc > 1 ? atoi(argv[1]) : 300;
  uint32_t s = 12345;
  auto rnd = [&s]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  std::vector<uint8_t> img, out;
  long long bytes = 0;
  for (int it = 0; it < iterations; ++it) {
    const int W = 1 + rnd() % 70, H = 1 + rnd() % 70, C = rnd() % 4 == 0 ? 1 : 3, sub = rnd() % 3;
    const int quality = it % 3 == 0 ? 100 : (it % 3 == 1 ? 1 : 1 + rnd() % 100);
    const int kind = rnd() % 4;                               // noise, extremes only, flat, stripes
    img.resize((size_t)W * H * C);
    const uint8_t flat = (uint8_t)rnd();
    for (size_t i = 0; i < img.size(); ++i)
      img[i] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? (uint8_t)((rnd() & 1) * 255) : kind == 2 ? flat : (uint8_t)((((i / C) % W) / 8 % 2) * 255);
    out.assign((size_t)JPEG_ENC_HEADER_MAX + 2 * (size_t)JPEG_ENC_BLOCK_BYTES * ((W + 15) / 8) * ((H + 15) / 8) * 3 + 2, 0);
    const int64_t n = jpeg_enc_host_encode(img.data(), H, W, C, quality, sub, out.data(), (int64_t)out.size());
    if (n < 4 || out[0] != 0xFF || out[1] != 0xD8 || out[n - 2] != 0xFF || out[n - 1] != 0xD9) {
      printf("iteration %d: %dx%d C=%d sub=%d q=%d -> %lld\n", it, W, H, C, sub, quality, (long long)n);
      return 1;
    }
    bytes += n;
  }
  printf("iterations %d, bytes %lld\n", iterations, bytes);
  return 0;
}
