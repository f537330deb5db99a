// full_search_host_loop.cc -- the per-picture loop that sjpeg_hip_encode_ragged_full_src replaces, for
// tools/ragged_full_time.py: sjpeg::Encode(EncoderParam) through the host API, one picture at a time from host memory.
//   full_search_host_loop CASES OUT_DIR
// CASES: one line per picture -- rgb_path width height quality method yuv_mode target_mode target passes tolerance.
// The first picture is coded once before the clock starts (device context, engine scratch).  Writes OUT_DIR/<line>.jpg
// and prints "loop_ms <milliseconds>" for all pictures together (file reads and writes outside the clock).
#include <stdio.h>

#include <chrono>
#include <string>
#include <vector>

#include "sjpeg.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* cases = fopen(argv[1], "r");
  if (cases == nullptr) return 2;
  char path[4096];
  int w, h, method, yuv, tmode, passes;
  float quality, target, tol;
  double ms = 0.;
  for (int line = 0; fscanf(cases, "%4095s %d %d %f %d %d %d %f %d %f", path, &w, &h, &quality, &method, &yuv, &tmode, &target,
                                   &passes, &tol) == 10; ++line) {
    std::vector<uint8_t> rgb(static_cast<size_t>(3) * w * h);
    FILE* f = fopen(path, "rb");
    if (f == nullptr || fread(rgb.data(), 1, rgb.size(), f) != rgb.size()) return 3;
    fclose(f);
    sjpeg::EncoderParam param(quality);
    param.yuv_mode = static_cast<SjpegYUVMode>(yuv);
    param.Huffman_compress = method != 0 && method != 3;
    param.adaptive_quantization = method >= 3;
    param.use_trellis = method >= 7;
    param.target_mode = tmode == 1 ? sjpeg::EncoderParam::TARGET_SIZE : sjpeg::EncoderParam::TARGET_PSNR;
    param.target_value = target;
    param.passes = passes;
    param.tolerance = tol;
    std::string out;
    for (int rep = (line == 0 ? 0 : 1); rep < 2; ++rep) {
      out.clear();
      const auto t0 = std::chrono::steady_clock::now();
      if (!sjpeg::Encode(rgb.data(), w, h, 3 * w, param, &out)) {
        fprintf(stderr, "line %d: %s\n", line, SjpegHipLastError());
        return 4;
      }
      if (rep == 1) ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const std::string name = std::string(argv[2]) + "/" + std::to_string(line) + ".jpg";
    FILE* o = fopen(name.c_str(), "wb");
    if (o == nullptr || fwrite(out.data(), 1, out.size(), o) != out.size()) return 5;
    fclose(o);
  }
  fclose(cases);
  printf("loop_ms %.3f\n", ms);
  return 0;
}
