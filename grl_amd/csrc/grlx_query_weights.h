// grlx_query_weights.h -- the non-creating table read of the policy queries (grlx_query.hip) and of the greedy evaluation episodes
// (grlx_evaluate.hip): the two units' common part.  Included after grlx_internal.h, grlx_rng.h and grlx_table.h; no rollout kernel sees it.
#pragma once

namespace grlx {

constexpr int kQueryWaves = 4;             // waves per block
constexpr int kRowStride = 66;             // doubles between two rows of a wave's LDS tile (grlx_query.hip, "LDS")

__device__ __forceinline__ double query_clamp(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// NP slots of one lane in `tab`: current weight, or the lazy initial value of a slot that has no entry.  Nothing is written.
template <int NP>
__device__ __forceinline__ void query_weights(const Table &tab, const ReplicaState &rs, int table, const LinearParams &lp,
                                              const uint32_t (&slot)[NP], double (&w)[NP])
{
  uint32_t b[NP], pos[NP];
  uint4 k[NP];
  bool hit[NP];
#pragma unroll
  for (int a = 0; a < NP; ++a)
  { // all key loads in flight before the first is used
    b[a] = table_home(tab, slot[a]);
    k[a] = bucket_keys(tab, b[a]);
  }
#pragma unroll
  for (int a = 0; a < NP; ++a)
  {
    uint32_t empty;
    int way = bucket_find(k[a], slot[a], empty);
    if (rarely(way < 0 && empty == 0u))
    { // home bucket full of other slots: walk on as table_peek does
      for (int it = 1; it < kMaxProbe; ++it)
      {
        b[a] = (b[a] + 1u) & tab.bmask;
        way = bucket_find(bucket_keys(tab, b[a]), slot[a], empty);
        if (way >= 0 || empty != 0u) break;
      }
    }
    hit[a] = way >= 0;
    pos[a] = (b[a] << 2) | (uint32_t)(way & 3);
  }
#pragma unroll
  for (int a = 0; a < NP; ++a) w[a] = hit[a] ? value_load(tab, pos[a]) : 0.;
#pragma unroll
  for (int a = 0; a < NP; ++a)
    if (!hit[a]) w[a] = initial_weight(rs, table, lp, slot[a]);
}

} // namespace grlx
