// grlx_host_rules.h -- the rules of the C ABI's host side that need nothing but integers and a grlx_config, each written once.
// HIP-free, so that tools/host_rules_check.cpp checks them as a program of its own; grlx_host.h holds the two constants below to
// grlx_internal.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/grlx.h"

namespace grlx {

constexpr size_t kRuleEntryBytes = 16;               // sizeof(Entry)
constexpr size_t kRuleTraceWords = 16 * 10 * 2;      // a replica's persisted trace: 16 lanes x kMaxTrace entries x (position, count | weight)

// host copy of the drand48-family LCG (utils.h:84-137), used only to seed the replicas
constexpr uint64_t kA = 0x5DEECE66DULL, kC = 0xBULL, kM = (1ULL << 48) - 1;
inline uint64_t h_seed(long s) { return ((((uint64_t)s) & 0xFFFFFFFFULL) << 16) | 0x330EULL; }   // srand48
inline uint64_t h_next(uint64_t x) { return (kA * x + kC) & kM; }
inline uint64_t h_jump(uint64_t x, uint64_t n)
{
  uint64_t a = kA, c = kC;
  while (n)
  {
    if (n & 1) x = (a * x + c) & kM;
    c = ((a + 1) * c) & kM;
    a = (a * a) & kM;
    n >>= 1;
  }
  return x;
}

// The growth rule of the sparse tables.  `used`: the slots of the fullest table.  Up to a quarter full the tables stay as they are; beyond,
// they grow until the fullest is at most an eighth full, bounded by logC_max.
inline uint32_t growth_target(uint32_t used, uint32_t logC, uint32_t logC_max)
{
  if ((uint64_t)used * 4u <= (1ull << logC)) return logC;
  uint32_t want = logC;
  while ((uint64_t)used * 8u > (1ull << want) && want < logC_max) ++want;
  return want;
}

// The distance on a replica's thread-local stream that the initial parameters cover (outputs = 1): the representation's table, the second
// table of the actor-critic and of QV, and the target network's own draws.  At create the stream is jumped by it from its seed.  At
// grlx_reset_run the walk of {action: reset} reaches the same objects in the order of construction (a provided target network is a child
// configurator, visited before the representation itself: configurable.cpp:690-712, 754-757; it draws again first, the representation
// next, synchronize() blends the two fresh vectors; ParameterizedRepresentation::count_ = 0), from the continuing stream.
inline uint64_t table_draws(const grlx_config &c)
{
  uint64_t draws = (uint64_t)c.projector.memory;
  if (c.agent == GRLX_AGENT_AC || c.agent == GRLX_AGENT_QV) draws += (uint64_t)c.actor_projector.memory;
  if (c.target_interval > 0) draws += (uint64_t)c.projector.memory;
  return draws;
}

// device bytes of n_tables tables of N replicas at 2^logC entries each, of the target values beside table 0, and the words of the persisted traces
inline size_t table_bytes(size_t N, size_t n_tables, uint32_t logC) { return (N * n_tables * kRuleEntryBytes) << logC; }
inline size_t tval_bytes(size_t N, uint32_t logC) { return (N * sizeof(double)) << logC; }
inline size_t trace_words(size_t N) { return N * kRuleTraceWords; }

// ---- what a projector admits: tile_quant casts floor(x * scaling) to int (tile_coding.cpp:121-125), so every coordinate of a projector's
// input must be finite with |x * scaling| < 2^30.  0: the rows [n, dims] are admitted; 1: *row, *dim name the first coordinate that is not
// finite; 2: the first whose product reaches 2^30 (a product that is not finite counts as reaching it).
constexpr double kRuleQuantBound = 1073741824.;      // 2^30
inline bool quant_admits(double x, double scaling)
{
  const double q = x * scaling;
  return x - x == 0. && (q < 0 ? -q : q) < kRuleQuantBound;      // x - x: 0 for finite x, NaN otherwise
}
inline int quant_admit_rows(const double *in, int n, int dims, const double *scaling, int *row, int *dim)
{
  for (int o = 0; o < n; ++o)
    for (int i = 0; i < dims; ++i)
    {
      const double x = in[(size_t)o * (size_t)dims + (size_t)i];
      if (quant_admits(x, scaling[i])) continue;
      *row = o;
      *dim = i;
      return x - x == 0. ? 2 : 1;
    }
  return 0;
}

// ---- streamed trajectories (grlx_evaluate_trajectory_stream): what one chunk stages, and how many start states a chunk holds
// The bytes one start state puts on the device, and the part of them that comes back: its state in (S doubles) and, for each of `rows`
// replicas, max_steps records of R doubles, ret, disc, the final state (S doubles) and steps, terminal, ties (int32).  The same count
// grlx_evaluate_trajectory bounds.
inline uint64_t stream_out_bytes(int rows, int max_steps, int R, int S)
{
  return (uint64_t)rows * ((uint64_t)max_steps * (uint64_t)R * 8u + 2u * 8u + (uint64_t)S * 8u + 3u * 4u);
}
inline uint64_t stream_start_bytes(int rows, int max_steps, int R, int S) { return (uint64_t)S * 8u + stream_out_bytes(rows, max_steps, R, S); }

// Two slots share the staging bound, so a chunk gets half of it (bound / 2, rounded down).  Start states per chunk: the largest count
// whose bytes fit the half, at most n_starts, and at most what one launch's grid takes -- a 16-lane group per (row, start state) pair,
// kRulePairsPerBlock pairs per block, 2^31 - 1 blocks.  -1: a single start state does not fit the half, and the call is refused.
constexpr uint64_t kRulePairsPerBlock = 16;          // 4 groups per wave x kQueryWaves waves
constexpr uint64_t kRuleMaxBlocks = 0x7fffffffull;
inline int stream_chunk(uint64_t bound, int rows, int max_steps, int R, int S, int n_starts)
{
  const uint64_t half = bound / 2, one = stream_start_bytes(rows, max_steps, R, S);
  if (one > half) return -1;
  uint64_t fit = half / one;
  if (rows > 0 && fit > kRuleMaxBlocks * kRulePairsPerBlock / (uint64_t)rows) fit = kRuleMaxBlocks * kRulePairsPerBlock / (uint64_t)rows;
  if (fit > (uint64_t)(n_starts < 0 ? 0 : n_starts)) fit = (uint64_t)(n_starts < 0 ? 0 : n_starts);
  return (int)fit;
}

} // namespace grlx
