// grlx_snapshot.h -- the two device kernels of a context snapshot (grlx_snapshot.hip), as the C-ABI layer launches them.
// They take everything as kernel arguments of their own: DevParams does not grow, and no rollout kernel sees this header.
#pragma once
#include "grlx_internal.h"
#include "grlx_snapshot_format.h"

namespace grlx {

// device-side error word of the two kernels
enum : uint32_t { SNAP_ERR_COUNT = 1u,      // pack: a table's occupied entries and ReplicaState::n_slots disagree
                  SNAP_ERR_RECORD = 2u };   // unpack: a record with an empty key, a position beyond the capacity, or out of order

// What both kernels work on.  Stream s = table * n_replicas + replica: `counts[s]` records beginning at record `offsets[s]` (the exclusive
// scan of the counts) of the record stream `records`, each `record_bytes` long (grlx_snapshot_format.h).
struct SnapshotArgs {
  Entry          *tables;        // [table][replica][2^logC]
  double         *tvals;         // [replica][2^logC] or null: the target network's value per position of table 0
  uint32_t        logC;
  int32_t         n_replicas, n_tables;
  const uint64_t *offsets;       // [n_tables * n_replicas]
  const uint32_t *counts;        // [n_tables * n_replicas]
  uint8_t        *records;
  uint32_t        record_bytes;
  uint32_t       *err;           // SNAP_ERR_* are or-ed in
};

// tables -> records: the occupied entries of every (table, replica), in ascending position
hipError_t launch_snapshot_pack(const SnapshotArgs &a, hipStream_t stream);
// records -> zeroed tables (tvals all ones): every record back at ITS position
hipError_t launch_snapshot_unpack(const SnapshotArgs &a, hipStream_t stream);

} // namespace grlx
