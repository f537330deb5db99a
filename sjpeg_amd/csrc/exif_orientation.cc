// exif_orientation.cc -- the EXIF Orientation (IFD0 tag 0x0112) of a picture's EXIF block, read and reset on the host
// (sjpeg_hip_exif_orientation, sjpeg_hip_exif_reset_orientation; sjpeg_hip.h).  Plain C++, no HIP: a host compiler
// builds this file alone (tests/cxx/exif_orientation_test.cc).  The payload is what sjpeg_hip_metadata.exif takes: an
// optional "Exif\0\0", then the TIFF header -- "II" 2A 00 or "MM" 00 2A, the offset of IFD0 --, IFD0 an entry count and
// entries of 12 bytes (tag, type, count, value).  Every read is checked against the size first.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sjpeg_hip.h"

namespace {

struct Tiff {
  const uint8_t* p;     // the TIFF header
  size_t n;             // bytes behind it
  bool big;             // "MM"
  bool has(size_t at, size_t len) const { return at <= n && len <= n - at; }
  uint32_t u16(size_t at) const { return big ? (p[at] << 8) | p[at + 1] : p[at] | (p[at + 1] << 8); }
  uint32_t u32(size_t at) const { return big ? (u16(at) << 16) | u16(at + 2) : u16(at) | (u16(at + 2) << 16); }
};

// Where the Orientation's value lies from `exif` and its byte order, when IFD0 has the tag as one SHORT; false for
// everything else.  The first entry with the tag decides.
bool find_orientation(const uint8_t* exif, size_t size, size_t* value_at, bool* big) {
  if (exif == nullptr) return false;
  size_t skip = 0;
  if (size >= 6 && memcmp(exif, "Exif\0\0", 6) == 0) skip = 6;
  Tiff t = {exif + skip, size - skip, false};
  if (!t.has(0, 8)) return false;
  if (t.p[0] == 'I' && t.p[1] == 'I') t.big = false;
  else if (t.p[0] == 'M' && t.p[1] == 'M') t.big = true;
  else return false;
  if (t.u16(2) != 42u) return false;
  const size_t ifd = t.u32(4);
  if (!t.has(ifd, 2)) return false;
  const size_t count = t.u16(ifd);
  for (size_t k = 0; k < count; ++k) {
    const size_t at = ifd + 2 + 12 * k;
    if (!t.has(at, 12)) return false;
    if (t.u16(at) != 0x0112u) continue;
    if (t.u16(at + 2) != 3u || t.u32(at + 4) != 1u) return false;      // SHORT, one of them
    *value_at = skip + at + 8;
    *big = t.big;
    return true;
  }
  return false;
}

}  // namespace

extern "C" {

int sjpeg_hip_exif_orientation(const uint8_t* exif, size_t size) {
  size_t at = 0;
  bool big = false;
  if (!find_orientation(exif, size, &at, &big)) return 0;
  const unsigned v = big ? (exif[at] << 8) | exif[at + 1] : exif[at] | (exif[at + 1] << 8);
  return v >= 1u && v <= 8u ? static_cast<int>(v) : 0;
}

int sjpeg_hip_exif_reset_orientation(uint8_t* exif, size_t size) {
  const int old = sjpeg_hip_exif_orientation(exif, size);
  if (old == 0) return 0;
  size_t at = 0;
  bool big = false;
  find_orientation(exif, size, &at, &big);
  exif[at] = big ? 0 : 1;
  exif[at + 1] = big ? 1 : 0;
  return old;
}

}  // extern "C"
