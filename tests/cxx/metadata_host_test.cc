// metadata_host_test.cc -- the host code behind per-picture metadata that needs no device (jpeg_host.cc: the checks and
// sizes of sjpeg_hip_metadata_size, the header assembly of the ragged calls), as a stand-alone program: built with
// -fsanitize=address,undefined by tests/test_ragged_meta_cxx.py and run on the CPU.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "jpeg_host.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main() {
  using namespace sjpeg_host;
  uint8_t quant[2][64];
  memset(quant, 16, sizeof(quant));
  const HuffSpec* dc[2] = {&DefaultHuff(0, 0), &DefaultHuff(0, 1)};
  const HuffSpec* ac[2] = {&DefaultHuff(1, 0), &DefaultHuff(1, 1)};
  std::vector<uint8_t> bare;
  CHECK(AppendHeaders(96, 64, SJPEG_HIP_YUV420, quant, dc, ac, nullptr, &bare));

  // every kind, sizes around the segment limits
  const std::string note = "<x:xmpmeta xmpNote:HasExtendedXMP=\"" + std::string(32, '0') + "\">";
  struct Case { size_t app, exif, iccp, xmp; uint16_t split; bool ok; const char* field; };
  const Case cases[] = {
      {0, 0, 0, 0, 0, true, ""},          {12, 0, 0, 0, 0, true, ""},        {0, 65527, 0, 0, 0, true, ""},
      {0, 65528, 0, 0, 0, false, "exif"}, {0, 0, 65519, 0, 0, true, ""},     {0, 0, 65520, 0, 0, true, ""},
      {0, 0, 1 << 20, 0, 0, true, ""},    {0, 0, 255 * 65519 + 1, 0, 0, false, "iccp"},
      {0, 0, 0, 65504, 0, true, ""},      {0, 0, 0, 65505, 0, true, ""},     {0, 0, 0, 200000, 0, true, ""},
      {0, 0, 0, 90000, 4000, true, ""},   {0, 0, 0, 90000, 30, false, "xmp"}, {7, 100, 3000, 500, 0, true, ""},
  };
  for (const Case& c : cases) {
    const std::string app(c.app, 'A'), exif(c.exif, 'E'), iccp(c.iccp, 'I');
    std::string xmp;
    if (c.xmp > 0) { xmp = note; xmp.resize(c.xmp, 'x'); }
    sjpeg_hip_metadata m;
    memset(&m, 0, sizeof(m));
    m.app_markers = app.data(); m.app_markers_size = app.size();
    m.exif = exif.data(); m.exif_size = exif.size();
    m.iccp = iccp.data(); m.iccp_size = iccp.size();
    m.xmp = xmp.data(); m.xmp_size = xmp.size();
    m.xmp_split_point = c.split;
    Metadata meta;
    std::vector<uint8_t> block;
    const char* field = "";
    const bool ok = MetadataFromC(&m, &meta, &block, &field);
    CHECK(ok == c.ok);
    if (!ok) { CHECK(std::string(field) == c.field); continue; }
    // the block is what AppendHeaders inserts behind SOI + APP0, and AppendHeadersBlock gives the same bytes
    std::vector<uint8_t> with, again;
    CHECK(AppendHeaders(96, 64, SJPEG_HIP_YUV420, quant, dc, ac, &meta, &with));
    CHECK(AppendHeadersBlock(96, 64, SJPEG_HIP_YUV420, quant, dc, ac, block.data(), block.size(), &again));
    CHECK(with == again);
    CHECK(with.size() == bare.size() + block.size());
    CHECK(memcmp(with.data(), bare.data(), 20) == 0);
    CHECK(block.empty() || memcmp(with.data() + 20, block.data(), block.size()) == 0);
    CHECK(memcmp(with.data() + 20 + block.size(), bare.data() + 20, bare.size() - 20) == 0);
    // (what the size search counts of it, HeaderSize(), is the reference's own estimate: not compared here)
    (void)SearchHeaderBits(3, 2, dc, ac, &meta);
  }
  // NULL is no metadata; a NULL member with a size is refused by name
  Metadata meta;
  std::vector<uint8_t> block(3, 1);
  const char* field = "";
  CHECK(MetadataFromC(nullptr, &meta, &block, &field) && block.empty());
  sjpeg_hip_metadata m;
  memset(&m, 0, sizeof(m));
  m.iccp_size = 4;
  CHECK(!MetadataFromC(&m, &meta, &block, &field) && std::string(field) == "iccp");
  // headers of several frames appended to one vector, as the ragged flows stage them
  std::vector<uint8_t> all;
  std::vector<uint8_t> blk(70000, 0x5a);
  size_t at = 0;
  for (int k = 0; k < 4; ++k) {
    CHECK(AppendHeadersBlock(17 + k, 13, k == 3 ? SJPEG_HIP_YUV400 : SJPEG_HIP_YUV444, quant, dc, ac, blk.data(), k * 23333, &all));
    CHECK(all.size() > at + 20 + static_cast<size_t>(k) * 23333);
    at = all.size();
  }
  printf("metadata host checks ok\n");
  return 0;
}
