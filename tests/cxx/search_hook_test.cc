// search_hook_test.cc -- what sjpeg::Encode's SearchHook holds after a searched encode (best q and best result), for
// tests/test_ragged_search.py: the batch search's q_out / value_out must be the same floats.
//   search_hook_test CASES OUT_DIR
// CASES: one line per picture -- rgb_path width height quality method yuv_mode target_mode target passes tolerance
// qmin qmax.  Writes OUT_DIR/<line>.jpg and prints "<line> <q> <value>" (%a: exact floats) per line.
#include <stdio.h>

#include <string>
#include <vector>

#include "sjpeg.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* cases = fopen(argv[1], "r");
  if (cases == nullptr) return 2;
  char path[4096];
  int w, h, method, yuv, tmode, passes;
  float quality, target, tol, qmin, qmax;
  for (int line = 0; fscanf(cases, "%4095s %d %d %f %d %d %d %f %d %f %f %f", path, &w, &h, &quality, &method, &yuv, &tmode,
                                   &target, &passes, &tol, &qmin, &qmax) == 12; ++line) {
    std::vector<uint8_t> rgb(static_cast<size_t>(3) * w * h);
    FILE* f = fopen(path, "rb");
    if (f == nullptr || fread(rgb.data(), 1, rgb.size(), f) != rgb.size()) return 3;
    fclose(f);
    sjpeg::EncoderParam param(quality);
    param.yuv_mode = static_cast<SjpegYUVMode>(yuv);
    param.Huffman_compress = method != 0 && method != 3;
    param.adaptive_quantization = method >= 3;
    param.target_mode = tmode == 1 ? sjpeg::EncoderParam::TARGET_SIZE : sjpeg::EncoderParam::TARGET_PSNR;
    param.target_value = target;
    param.passes = passes;
    param.tolerance = tol;
    param.qmin = qmin;
    param.qmax = qmax;
    sjpeg::SearchHook hook;
    param.search_hook = &hook;
    std::string out;
    if (!sjpeg::Encode(rgb.data(), w, h, 3 * w, param, &out)) {
      fprintf(stderr, "line %d: %s\n", line, SjpegHipLastError());
      return 4;
    }
    const std::string name = std::string(argv[2]) + "/" + std::to_string(line) + ".jpg";
    FILE* o = fopen(name.c_str(), "wb");
    if (o == nullptr || fwrite(out.data(), 1, out.size(), o) != out.size()) return 5;
    fclose(o);
    printf("%d %a %a\n", line, hook.q, hook.value);
  }
  fclose(cases);
  return 0;
}
