// grlx_snapshot_format.h -- the byte layout of a context snapshot (grlx_snapshot_save / _load / _info) and the reader / writer of
// its header.  HIP-free on purpose: this pair compiles alone with any C++17 compiler (tools/snapshot_format_check.cpp does, under
// the host sanitizers), and nothing here touches a device.
//
// A snapshot is ONE little-endian byte string:
//
//   header   kFixedBytes (128) of fields, then the grlx_config the context was created with (its own struct_size first), zero-padded
//            to a multiple of 16:
//              0   char[8]  magic "GRLXSNAP"
//              8   u32      format version (kVersion)
//              12  u32      header bytes (fields + configuration + padding)
//              16  u64      total bytes of the snapshot
//              24  u64      payload checksum: FNV-1a 64 (offset basis 0xcbf29ce484222325, prime 0x100000001b3) over every byte after the header
//              32  u64      header checksum: the same function over the header with these eight bytes taken as zero
//              40  u32      n_replicas        44  u32  n_tables          48  u32  logC (table entries per replica and table = 2^logC)
//              52  u32      flags (kFlag*)    56  i64  trials_run        64  u32  rows (largest ReplicaState::rows of the context)
//              68  u32      record bytes      72  u64  section bytes [5] (states, rows, trace, sweep, records)
//              112 u64      records in the record section
//              120 u32      bytes of one ReplicaState (kStateBytes)      124 u32  GRLX_ABI_VERSION
//   sections, in this order, each directly behind the one before (all sizes are multiples of 8):
//     states   ReplicaState[n_replicas] as the device holds them, with the three device pointers (lazy_base[2], target_base) written as zero
//     rows     row_reward[rows][n_replicas] f64, row_time[..] f64, row_steps[..] i64, row_trial[..] i64; a slot at or above its replica's own
//              ReplicaState::rows (ragged counts under a steps budget; an earlier run's rows after grlx_reset_run) is written as zero
//     trace    the actor-critic's persisted critic trace, u32 [n_replicas][16][10][2]              (kFlagTrace)
//     sweep    the per-replica values f64 [4][n_replicas]: alpha, gamma, lambda, epsilon           (kFlagSweep)
//     records  per (table, replica) in ascending table, then replica, then POSITION order one record per occupied entry:
//                u32 position | u32 key word | u32 aux (claim) word | u32 zero | f64 value [| f64 target value]
//              24 bytes, or 32 with a target network (kFlagTarget; the target value of table 0's position, the all-ones "not
//              materialised" pattern kept as it is).  The count of stream (t, r) is ReplicaState[r].n_slots[t].
//
// Twin tables (actor-critic with equal tile codings, kFlagTwin): the two tables hold the same key at the same position.  They are
// written as what they are -- two streams, each with its own key, aux and value words -- and because a restore puts every record
// back at ITS position, the pair comes back at equal positions without a word about it in the file.
//
// The order is canonical: two contexts in the same state give the same bytes (apart from the configuration block where their
// layout fields differ).  A snapshot holds no device pointer and nothing that lives inside one launch only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/grlx.h"

namespace grlx {
namespace snap {

constexpr char     kMagic[8] = {'G', 'R', 'L', 'X', 'S', 'N', 'A', 'P'};
constexpr uint32_t kVersion = 1;
constexpr uint32_t kFixedBytes = 128;
constexpr uint32_t kStateBytes = 256;                      // sizeof(ReplicaState), checked where that type is known
constexpr uint32_t kStatePointerOffsets[3] = {216, 224, 248};   // lazy_base[0], lazy_base[1], target_base
constexpr uint32_t kStateSlotsOffset = 184, kStateRowsOffset = 196;     // n_slots[2], rows
constexpr uint32_t kTraceWordsPerReplica = 16 * 10 * 2;
constexpr uint32_t kRecordBytes = 24, kRecordBytesTarget = 32;
enum : uint32_t { kFlagSweep = 1u, kFlagTrace = 2u, kFlagTarget = 4u, kFlagTwin = 8u, kFlagsKnown = 15u };
enum { SEC_STATES = 0, SEC_ROWS = 1, SEC_TRACE = 2, SEC_SWEEP = 3, SEC_RECORDS = 4, SEC_COUNT = 5 };

struct Header {
  uint32_t version, header_bytes;
  uint64_t total_bytes, checksum;
  uint32_t n_replicas, n_tables, logC, flags;
  int64_t  trials_run;
  uint32_t rows, record_bytes;
  uint64_t section_bytes[SEC_COUNT];
  uint64_t n_records;
  grlx_config cfg;
};

uint64_t fnv1a(const void *data, size_t bytes, uint64_t h = 0xcbf29ce484222325ull);
uint32_t header_bytes();
// section sizes, record size and total size from the counts of `h` (n_replicas, n_tables, flags, rows, n_records)
void fill_sizes(Header *h);
// out: header_bytes() bytes.  h.checksum is written as given; the header checksum is computed here.
void write_header(const Header &h, uint8_t *out);
// 0, or -1 with the reason in msg: everything that can be said about a header without the rest of the file.  `bytes` may be the
// header alone; a buffer shorter than its header, or any byte of the header altered, is refused.
int read_header(const void *buf, uint64_t bytes, Header *out, char *msg, size_t msg_cap);

} // namespace snap
} // namespace grlx
