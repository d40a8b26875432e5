// snapshot_format_check.cpp -- stand-alone check of the snapshot header's reader (grl_amd/csrc/grlx_snapshot_format.{h,cpp}): host code
// only, meant to be compiled with the host sanitizers, e.g.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/snapshot_format_check.cpp grl_amd/csrc/grlx_snapshot_format.cpp -o check
// It writes a valid header, then reads it back truncated at every length and with every byte altered once: every malformed input must
// be refused, with a message, and nothing may be read outside the buffer handed in (each case gets a heap buffer of exactly its length).
// `snapshot_format_check FILE` also writes the valid header to FILE (tests/test_snapshot_host.py feeds it to grlx_snapshot_info).
#include <cstdio>
#include <cstring>
#include <vector>
#include "../grl_amd/csrc/grlx_snapshot_format.h"

using namespace grlx::snap;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

static int read_exact(const uint8_t *src, size_t n, Header *out, char *msg, size_t cap)
{
  std::vector<uint8_t> exact(src, src + n);          // a buffer of exactly n bytes: one byte too far is a heap overflow the sanitizer sees
  return read_header(n ? exact.data() : (const uint8_t *)"", n, out, msg, cap);
}

int main(int argc, char **argv)
{
  Header h;
  memset(&h, 0, sizeof(h));
  h.cfg.struct_size = sizeof(grlx_config);
  h.cfg.n_replicas = 13;
  h.cfg.max_rows = 24;
  h.cfg.alpha = 0.2;
  h.n_replicas = 13;
  h.n_tables = 2;
  h.logC = 13;
  h.flags = kFlagTrace | kFlagTwin;
  h.trials_run = 12;
  h.rows = 1;
  h.n_records = 4321;
  h.checksum = 0x0123456789abcdefull;
  fill_sizes(&h);
  const uint32_t hb = header_bytes();
  EXPECT(h.header_bytes == hb && hb % 16 == 0 && hb >= kFixedBytes + sizeof(grlx_config), "header size %u", hb);
  std::vector<uint8_t> good(hb);
  write_header(h, good.data());
  if (argc > 1)
  {
    FILE *f = fopen(argv[1], "wb");
    if (!f || fwrite(good.data(), 1, good.size(), f) != good.size()) { fprintf(stderr, "cannot write %s\n", argv[1]); return 2; }
    fclose(f);
  }
  Header back;
  char msg[256];
  msg[0] = 0;
  EXPECT(read_exact(good.data(), hb, &back, msg, sizeof(msg)) == 0, "the valid header is refused: %s", msg);
  EXPECT(back.total_bytes == h.total_bytes && back.n_records == h.n_records && back.trials_run == 12 && back.flags == h.flags && back.logC == 13 &&
         back.checksum == h.checksum && memcmp(&back.cfg, &h.cfg, sizeof(grlx_config)) == 0, "the header does not read back as written");
  for (size_t n = 0; n < hb; ++n)
  { // truncated at every length
    msg[0] = 0;
    EXPECT(read_exact(good.data(), n, &back, msg, sizeof(msg)) != 0, "a header cut at %zu bytes is accepted", n);
    EXPECT(msg[0] != 0, "no message for a header cut at %zu bytes", n);
  }
  for (size_t i = 0; i < hb; ++i)
    for (uint8_t flip : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF})
    { // every byte altered once (three ways)
      std::vector<uint8_t> bad(good);
      bad[i] ^= flip;
      msg[0] = 0;
      EXPECT(read_exact(bad.data(), hb, &back, msg, sizeof(msg)) != 0, "byte %zu ^ 0x%02x is accepted", i, flip);
      EXPECT(msg[0] != 0, "no message for byte %zu ^ 0x%02x", i, flip);
    }
  { // a newer format version, with a header checksum that is right for it: refused for the version
    Header newer = h;
    std::vector<uint8_t> buf(hb);
    write_header(newer, buf.data());
    const uint32_t v = kVersion + 1;
    memcpy(buf.data() + 8, &v, 4);
    msg[0] = 0;
    EXPECT(read_exact(buf.data(), hb, &back, msg, sizeof(msg)) != 0 && strstr(msg, "newer") != nullptr, "a newer format version: '%s'", msg);
  }
  { // counts that do not add up, under a valid header checksum
    Header wrong = h;
    wrong.section_bytes[SEC_RECORDS] += 24;
    std::vector<uint8_t> buf(hb);
    write_header(wrong, buf.data());
    EXPECT(read_exact(buf.data(), hb, &back, msg, sizeof(msg)) != 0, "a record section that disagrees with its count is accepted");
    wrong = h;
    wrong.n_records = (2ull * 13ull << 13) + 1;
    fill_sizes(&wrong);
    write_header(wrong, buf.data());
    EXPECT(read_exact(buf.data(), hb, &back, msg, sizeof(msg)) != 0, "more records than the tables hold are accepted");
    wrong = h;
    wrong.logC = 27;
    write_header(wrong, buf.data());
    EXPECT(read_exact(buf.data(), hb, &back, msg, sizeof(msg)) != 0, "a capacity of 2^27 is accepted");
  }
  EXPECT(read_header(nullptr, 100, &back, msg, sizeof(msg)) != 0, "a null buffer is accepted");
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("snapshot format: %u-byte header, %u truncations and %u altered bytes refused\n", hb, hb, 3 * hb);
  return 0;
}
