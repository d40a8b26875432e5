// grlx_snapshot.hip -- the device side of a context snapshot: the sparse tables compacted into a canonical record stream, and back.
// A translation unit of its own (like grlx_fqi.hip): no rollout kernel is compiled with it, so none of them changes.
//
// A table is 2^(logC-2) buckets of 64 bytes (grlx_table.h: Bucket = key[4] | aux[4] | val[4]), position = bucket * 4 + way, and a
// run leaves most of them empty.  A snapshot keeps the occupied entries only, in ascending position, so that two contexts in the
// same state give the same bytes; a restore puts every record back at ITS position (the persisted critic trace, the target values
// and twin tables refer to positions), never re-hashes.
#include "grlx_internal.h"
#include "grlx_snapshot.h"

namespace grlx {

namespace {

constexpr uint32_t kSnapKeyMask = 0x03FFFFFFu;        // kKeyMask of grlx_table.h: the slot bits of a key word, 0 = empty

// a bucket as four 16-byte quads: keys, aux words, values 0-1, values 2-3
__device__ __forceinline__ const uint4 *bucket_quads(const Entry *table, uint32_t b) { return reinterpret_cast<const uint4 *>(table) + (size_t)b * 4u; }

__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t o = __shfl_up(v, d, 64);
    v += lane >= d ? o : 0u;
  }
  return v;
}

} // namespace

// One wave per stream (table, replica).  Per pass every lane loads the key quad of one bucket of each of four consecutive 64-bucket
// groups (four 16-byte loads in flight per lane), counts its occupied ways, takes the prefix over the wave and adds the base carried
// from the groups before: that is the record index of its first entry, and records come out in ascending position.  Only occupied ways
// load their aux word and value.  A record index at or beyond the stream's count is not written (the stream never leaves its section);
// a total that differs from the count raises SNAP_ERR_COUNT.
__global__ __launch_bounds__(64) void snapshot_pack_kernel(SnapshotArgs a)
{
  const uint32_t s = blockIdx.x;
  const int lane = threadIdx.x;
  const Entry *table = a.tables + ((size_t)s << a.logC);
  const double *tvals = (a.tvals && s < (uint32_t)a.n_replicas) ? a.tvals + ((size_t)s << a.logC) : nullptr;      // table 0 only
  const uint32_t count = a.counts[s], rb = a.record_bytes;
  uint8_t *out = a.records + a.offsets[s] * rb;
  const uint32_t n_buckets = 1u << (a.logC - 2);
  uint32_t base = 0;
  for (uint32_t b0 = 0; b0 < n_buckets; b0 += 256u)
  {
    uint4 k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const uint32_t b = b0 + 64u * j + lane;
      k[j] = b < n_buckets ? *bucket_quads(table, b) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const uint32_t b = b0 + 64u * j + lane;
      const uint32_t kw[4] = {k[j].x, k[j].y, k[j].z, k[j].w};
      uint32_t n = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) n += (kw[w] & kSnapKeyMask) != 0u ? 1u : 0u;
      const uint32_t incl = wave_inclusive_sum(n, lane);
      uint32_t idx = base + incl - n;
      if (n != 0u)
      {
        const uint32_t *aux = reinterpret_cast<const uint32_t *>(bucket_quads(table, b) + 1);
        const double *val = reinterpret_cast<const double *>(bucket_quads(table, b) + 2);
#pragma unroll
        for (int w = 0; w < 4; ++w)
          if ((kw[w] & kSnapKeyMask) != 0u)
          {
            if (idx < count)
            {
              const uint32_t pos = (b << 2) | (uint32_t)w;
              uint8_t *rec = out + (size_t)idx * rb;
              *reinterpret_cast<uint2 *>(rec) = make_uint2(pos, kw[w]);
              *reinterpret_cast<uint2 *>(rec + 8) = make_uint2(aux[w], 0u);
              *reinterpret_cast<double *>(rec + 16) = val[w];
              if (rb == snap::kRecordBytesTarget)
                *reinterpret_cast<unsigned long long *>(rec + 24) = tvals ? reinterpret_cast<const unsigned long long *>(tvals)[pos] : ~0ull;
            }
            ++idx;
          }
      }
      base += __shfl(incl, 63, 64);
    }
  }
  if (lane == 0 && base != count) atomicOr(a.err, SNAP_ERR_COUNT);
}

// The inverse, into zeroed tables (target values all ones): the lanes of the stream's wave take its records in turn.  The position
// is masked into the replica's own table exactly as value_store / entry_create mask theirs (grlx_table.h), after the check that
// refuses it: whatever the file says, no access leaves the allocation.
__global__ __launch_bounds__(64) void snapshot_unpack_kernel(SnapshotArgs a)
{
  const uint32_t s = blockIdx.x;
  Entry *table = a.tables + ((size_t)s << a.logC);
  double *tvals = (a.tvals && s < (uint32_t)a.n_replicas) ? a.tvals + ((size_t)s << a.logC) : nullptr;
  const uint32_t count = a.counts[s], rb = a.record_bytes;
  const uint8_t *in = a.records + a.offsets[s] * rb;
  const uint32_t pmask = (1u << a.logC) - 1u;
  for (uint32_t i = threadIdx.x; i < count; i += 64u)
  {
    const uint8_t *rec = in + (size_t)i * rb;
    const uint2 pk = *reinterpret_cast<const uint2 *>(rec);
    const uint2 az = *reinterpret_cast<const uint2 *>(rec + 8);
    const double v = *reinterpret_cast<const double *>(rec + 16);
    const bool ordered = i == 0u || *reinterpret_cast<const uint32_t *>(rec - rb) < pk.x;
    if ((pk.y & kSnapKeyMask) == 0u || pk.x > pmask || az.y != 0u || !ordered)
    {
      atomicOr(a.err, SNAP_ERR_RECORD);
      continue;
    }
    const uint32_t pos = pk.x & pmask;
    uint32_t *bucket = reinterpret_cast<uint32_t *>(table) + (size_t)(pos >> 2) * 16u;
    bucket[pos & 3u] = pk.y;
    bucket[4u + (pos & 3u)] = az.x;
    reinterpret_cast<double *>(bucket + 8)[pos & 3u] = v;
    if (tvals && rb == snap::kRecordBytesTarget)
      reinterpret_cast<unsigned long long *>(tvals)[pos] = *reinterpret_cast<const unsigned long long *>(rec + 24);
  }
}

hipError_t launch_snapshot_pack(const SnapshotArgs &a, hipStream_t stream)
{
  hipLaunchKernelGGL(snapshot_pack_kernel, dim3((unsigned)(a.n_tables * a.n_replicas)), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_snapshot_unpack(const SnapshotArgs &a, hipStream_t stream)
{
  hipLaunchKernelGGL(snapshot_unpack_kernel, dim3((unsigned)(a.n_tables * a.n_replicas)), dim3(64), 0, stream, a);
  return hipGetLastError();
}

} // namespace grlx
