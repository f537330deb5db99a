// sjpeg_hip_exif_orientation / sjpeg_hip_exif_reset_orientation (sjpeg_amd/csrc/exif_orientation.cc, built with this
// file by the host compiler alone) on the payloads of tests/golden/exif_orientation.json, handed over as a text file:
// a line "<expected orientation> <hex of the payload> <hex after the reset>" each ("-" for an empty payload).  Every
// payload, every truncation of it and every single-byte change of its first 64 bytes goes into a heap buffer of exactly
// its size: under -fsanitize=address,undefined a read outside it ends the program.  A stand-alone program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sjpeg_hip.h"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(static_cast<uint8_t>(strtoul(s.substr(i, 2).c_str(), nullptr, 16)));
  return out;
}

// the two calls on a heap copy of exactly n bytes; -1 when an answer is out of range or the reset is inconsistent
static int both(const uint8_t* p, size_t n, std::vector<uint8_t>* after) {
  uint8_t* const q = n ? static_cast<uint8_t*>(malloc(n)) : nullptr;   // (an empty payload: nothing may be read at all)
  if (n) memcpy(q, p, n);
  const int o = sjpeg_hip_exif_orientation(q, n);
  const int old = sjpeg_hip_exif_reset_orientation(q, n);
  int rc = o;
  if (o < 0 || o > 8 || old != o) rc = -1;
  if (o != 0 && sjpeg_hip_exif_orientation(q, n) != 1) rc = -1;
  if (o == 0 && n && memcmp(q, p, n) != 0) rc = -1;                 // nothing found: nothing changed
  if (after != nullptr && n) after->assign(q, q + n);
  if (after != nullptr && !n) after->clear();
  free(q);
  return rc;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* const f = fopen(argv[1], "r");
  if (f == nullptr) return 2;
  static char line[1 << 16];
  long payloads = 0, tried = 0;
  while (fgets(line, sizeof(line), f) != nullptr) {
    int want = -1;
    char a[1 << 15], b[1 << 15];
    if (sscanf(line, "%d %32767s %32767s", &want, a, b) != 3) continue;
    const std::vector<uint8_t> p = unhex(a), reset = unhex(b);
    std::vector<uint8_t> after;
    if (both(p.data(), p.size(), &after) != want || after != reset) {
      printf("FAILED payload %ld: orientation or reset differs from the fixture\n", payloads);
      return 1;
    }
    ++payloads;
    for (size_t n = 0; n < p.size(); ++n, ++tried) {
      if (both(p.data(), n, nullptr) < 0) { printf("FAILED payload %ld cut to %zu\n", payloads - 1, n); return 1; }
    }
    std::vector<uint8_t> m = p;
    for (size_t i = 0; i < m.size() && i < 64; ++i) {
      for (int v = 0; v < 256; ++v, ++tried) {
        m[i] = static_cast<uint8_t>(v);
        if (both(m.data(), m.size(), nullptr) < 0) { printf("FAILED payload %ld byte %zu = %d\n", payloads - 1, i, v); return 1; }
      }
      m[i] = p[i];
    }
  }
  fclose(f);
  printf("exif orientation ok: %ld payloads, %ld variants\n", payloads, tried);
  return 0;
}
