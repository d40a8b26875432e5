// grlx_snapshot_format.cpp -- writer and reader of a snapshot's header (layout: grlx_snapshot_format.h).  No HIP, no device.
#include "grlx_snapshot_format.h"
#include <cstdio>
#include <cstring>

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "snapshots are little-endian and written from memory as it is");

namespace grlx {
namespace snap {

uint64_t fnv1a(const void *data, size_t bytes, uint64_t h)
{
  const uint8_t *p = (const uint8_t *)data;
  for (size_t i = 0; i < bytes; ++i)
  {
    h ^= p[i];
    h *= 0x100000001b3ull;
  }
  return h;
}

uint32_t header_bytes() { return kFixedBytes + (((uint32_t)sizeof(grlx_config) + 15u) & ~15u); }

void fill_sizes(Header *h)
{
  const uint64_t N = h->n_replicas;
  h->version = kVersion;
  h->header_bytes = header_bytes();
  h->record_bytes = (h->flags & kFlagTarget) ? kRecordBytesTarget : kRecordBytes;
  h->section_bytes[SEC_STATES] = N * kStateBytes;
  h->section_bytes[SEC_ROWS] = 4ull * 8ull * h->rows * N;
  h->section_bytes[SEC_TRACE] = (h->flags & kFlagTrace) ? N * kTraceWordsPerReplica * 4ull : 0ull;
  h->section_bytes[SEC_SWEEP] = (h->flags & kFlagSweep) ? 4ull * 8ull * N : 0ull;
  h->section_bytes[SEC_RECORDS] = h->n_records * h->record_bytes;
  h->total_bytes = h->header_bytes;
  for (int s = 0; s < SEC_COUNT; ++s) h->total_bytes += h->section_bytes[s];
}

namespace {
template <typename T> void put(uint8_t *out, size_t at, T v) { memcpy(out + at, &v, sizeof(T)); }
template <typename T> T get(const uint8_t *in, size_t at) { T v; memcpy(&v, in + at, sizeof(T)); return v; }
constexpr size_t kAtHeaderChecksum = 32;

uint64_t header_checksum(const uint8_t *hdr, uint32_t bytes)
{
  static const uint8_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t h = fnv1a(hdr, kAtHeaderChecksum);
  h = fnv1a(zero, 8, h);
  return fnv1a(hdr + kAtHeaderChecksum + 8, bytes - kAtHeaderChecksum - 8, h);
}

int refuse(char *msg, size_t cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0)
{
  if (msg && cap) snprintf(msg, cap, fmt, a, b);
  return -1;
}
} // namespace

void write_header(const Header &h, uint8_t *out)
{
  memset(out, 0, h.header_bytes);
  memcpy(out, kMagic, 8);
  put<uint32_t>(out, 8, h.version);
  put<uint32_t>(out, 12, h.header_bytes);
  put<uint64_t>(out, 16, h.total_bytes);
  put<uint64_t>(out, 24, h.checksum);
  put<uint32_t>(out, 40, h.n_replicas);
  put<uint32_t>(out, 44, h.n_tables);
  put<uint32_t>(out, 48, h.logC);
  put<uint32_t>(out, 52, h.flags);
  put<int64_t>(out, 56, h.trials_run);
  put<uint32_t>(out, 64, h.rows);
  put<uint32_t>(out, 68, h.record_bytes);
  for (int s = 0; s < SEC_COUNT; ++s) put<uint64_t>(out, 72 + 8 * (size_t)s, h.section_bytes[s]);
  put<uint64_t>(out, 112, h.n_records);
  put<uint32_t>(out, 120, kStateBytes);
  put<uint32_t>(out, 124, (uint32_t)GRLX_ABI_VERSION);
  memcpy(out + kFixedBytes, &h.cfg, sizeof(grlx_config));
  put<uint64_t>(out, kAtHeaderChecksum, header_checksum(out, h.header_bytes));
}

int read_header(const void *buf, uint64_t bytes, Header *out, char *msg, size_t cap)
{
  const uint8_t *in = (const uint8_t *)buf;
  if (!in || !out) return refuse(msg, cap, "snapshot: null argument");
  if (bytes < 16) return refuse(msg, cap, "snapshot: %llu bytes are not a snapshot (no room for the magic and the version)", bytes);
  if (memcmp(in, kMagic, 8) != 0) return refuse(msg, cap, "snapshot: bad magic (not a grlx snapshot)");
  Header h;
  memset(&h, 0, sizeof(h));
  h.version = get<uint32_t>(in, 8);
  if (h.version > kVersion) return refuse(msg, cap, "snapshot: format version %llu is newer than this library reads (%llu)", h.version, kVersion);
  if (h.version != kVersion) return refuse(msg, cap, "snapshot: format version %llu is not supported (this library reads %llu)", h.version, kVersion);
  h.header_bytes = get<uint32_t>(in, 12);
  if (h.header_bytes != header_bytes())
    return refuse(msg, cap, "snapshot: header of %llu bytes, this library's is %llu (another grlx_config)", h.header_bytes, header_bytes());
  if (bytes < h.header_bytes) return refuse(msg, cap, "snapshot: cut short inside the header (%llu of %llu bytes)", bytes, h.header_bytes);
  if (get<uint64_t>(in, kAtHeaderChecksum) != header_checksum(in, h.header_bytes)) return refuse(msg, cap, "snapshot: header checksum mismatch (the header is damaged)");
  h.total_bytes = get<uint64_t>(in, 16);
  h.checksum = get<uint64_t>(in, 24);
  h.n_replicas = get<uint32_t>(in, 40);
  h.n_tables = get<uint32_t>(in, 44);
  h.logC = get<uint32_t>(in, 48);
  h.flags = get<uint32_t>(in, 52);
  h.trials_run = get<int64_t>(in, 56);
  h.rows = get<uint32_t>(in, 64);
  h.record_bytes = get<uint32_t>(in, 68);
  for (int s = 0; s < SEC_COUNT; ++s) h.section_bytes[s] = get<uint64_t>(in, 72 + 8 * (size_t)s);
  h.n_records = get<uint64_t>(in, 112);
  memcpy(&h.cfg, in + kFixedBytes, sizeof(grlx_config));
  // the header is what its writer wrote (checksum); what follows guards against a writer of another build
  if (get<uint32_t>(in, 120) != kStateBytes) return refuse(msg, cap, "snapshot: replica state of %llu bytes, this library's has %llu", get<uint32_t>(in, 120), kStateBytes);
  if (get<uint32_t>(in, 124) != (uint32_t)GRLX_ABI_VERSION) return refuse(msg, cap, "snapshot: written by ABI version %llu, this library is %llu", get<uint32_t>(in, 124), GRLX_ABI_VERSION);
  if (h.cfg.struct_size != sizeof(grlx_config)) return refuse(msg, cap, "snapshot: grlx_config.struct_size %llu != %llu", h.cfg.struct_size, sizeof(grlx_config));
  if (h.n_replicas < 1 || h.n_replicas > 0x7FFFFFFFu || (int64_t)h.n_replicas != (int64_t)h.cfg.n_replicas)
    return refuse(msg, cap, "snapshot: n_replicas %llu disagrees with its configuration", h.n_replicas);
  if (h.n_tables < 1 || h.n_tables > 2) return refuse(msg, cap, "snapshot: n_tables %llu", h.n_tables);
  if (h.logC < 8 || h.logC > 26) return refuse(msg, cap, "snapshot: table capacity 2^%llu is outside 2^8..2^26", h.logC);
  if (h.flags & ~kFlagsKnown) return refuse(msg, cap, "snapshot: unknown flags %llu", h.flags);
  if (h.trials_run < 0) return refuse(msg, cap, "snapshot: negative trial count");
  if (h.cfg.max_rows < 1 || (int64_t)h.rows > (int64_t)h.cfg.max_rows) return refuse(msg, cap, "snapshot: %llu rows, the configuration reserves %llu", h.rows, (unsigned long long)h.cfg.max_rows);
  if (h.n_records > ((uint64_t)h.n_tables * h.n_replicas << h.logC)) return refuse(msg, cap, "snapshot: %llu records exceed the tables' capacity", h.n_records);
  Header want = h;
  fill_sizes(&want);
  if (h.record_bytes != want.record_bytes) return refuse(msg, cap, "snapshot: record size %llu, expected %llu", h.record_bytes, want.record_bytes);
  for (int s = 0; s < SEC_COUNT; ++s)
    if (h.section_bytes[s] != want.section_bytes[s])
      return refuse(msg, cap, "snapshot: a section holds %llu bytes where its counts give %llu", h.section_bytes[s], want.section_bytes[s]);
  if (h.total_bytes != want.total_bytes) return refuse(msg, cap, "snapshot: total size %llu, the sections add up to %llu", h.total_bytes, want.total_bytes);
  *out = h;
  return 0;
}

} // namespace snap
} // namespace grlx
