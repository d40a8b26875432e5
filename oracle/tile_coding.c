/* tile_coding.c -- hashed tile coding, restated (TEST INFRASTRUCTURE).
 *
 * Follows base/src/projectors/tile_coding.cpp:45-80 (configure: scaling,
 * integer wrapping), :103-149 (_project) and
 * base/include/grl/projectors/tile_coding.h:78-118 (MurmurHash2 over the
 * coordinate tuple with seed 449, index = hash % memory) and :116-151 (getFeatureLocation: the claim table of safe = 1 / 2,
 * orc_tile_claim below, which the experiments walk their table with).
 *
 * PINNED by the reference's own tile_coding.cpp and tile_coding.h, compiled unmodified into oracle/_ref/ref_tiles (oracle/ref):
 * tests/test_oracle_ref_tiles.py holds orc_tile_project, orc_tile_project_hash and orc_tile_claim to that binary index by index
 * on 1 to 8 dimensions, 1 to 32 tilings, wrapping on any dimension, memories that are no power of two, negative coordinates and
 * inputs on tile edges, and the specs configure() refuses; the golden learning curve pins the pendulum's projector besides.
 */
#include <math.h>
#include "oracle.h"

static int smod(int x, int y)
{ /* utils.h:70-78 safe_mod: C remainder lifted into [0, y) */
  int r = x % y;
  return r < 0 ? r + y : r;
}

static uint32_t murmur2_ints(const int *v, uint32_t n, uint32_t seed)
{ /* tile_coding.h:78-114: MurmurHash2 (Appleby), 4 bytes per coordinate */
  const uint32_t m = 0x5bd1e995u;
  uint32_t h = seed ^ n;
  for (uint32_t i = 0; i < n; ++i)
  {
    uint32_t k = (uint32_t)v[i];
    k *= m;
    k ^= k >> 24;
    k *= m;
    h *= m;
    h ^= k;
  }
  h ^= h >> 13;
  h *= m;
  h ^= h >> 15;
  return h;
}

static int tile_project_impl(const orc_tile_spec *t, const double *in, uint32_t *out, int full_hash);

int orc_tile_project(const orc_tile_spec *t, const double *in, uint32_t *out) { return tile_project_impl(t, in, out, 0); }
/* the same with the full 32-bit hash sums (createHashSum, tile_coding.h:78-113) instead of `% memory`: what the collision
 * table of safe >= 1 keys its claims with (getFeatureLocation, tile_coding.h:116-151) */
int orc_tile_project_hash(const orc_tile_spec *t, const double *in, uint32_t *out) { return tile_project_impl(t, in, out, 1); }

static int tile_project_impl(const orc_tile_spec *t, const double *in, uint32_t *out, int full_hash)
{
  int q[ORC_MAX_DIMS], base[ORC_MAX_DIMS], wrap[ORC_MAX_DIMS], c[ORC_MAX_DIMS + 1];
  double scaling[ORC_MAX_DIMS];
  int D = t->dims;

  if (D < 1 || D > ORC_MAX_DIMS || t->tilings < 1 || t->memory < 1)
    return -1;

  for (int i = 0; i < D; ++i)
  { /* tile_coding.cpp:66-78 */
    scaling[i] = t->tilings / t->resolution[i];
    double w = t->wrapping[i] * scaling[i];
    if (fabs(w - round(w)) > 0.001)
      return -1;
    wrap[i] = (int)round(w);
  }

  for (int i = 0; i < D; ++i)
  { /* :121-125 */
    q[i] = (int)floor(in[i] * scaling[i]);
    base[i] = 0;
  }

  for (int j = 0; j < t->tilings; ++j)
  { /* :128-146 */
    int i;
    for (i = 0; i < D; ++i)
    {
      c[i] = q[i] - smod(q[i] - base[i], t->tilings);
      if (wrap[i] != 0)
        c[i] = smod(c[i], wrap[i]);
      base[i] += 1 + 2 * i;
    }
    c[i] = j;
    /* tile_coding.h:118: unsigned % int -> unsigned arithmetic */
    out[j] = murmur2_ints(c, (uint32_t)(D + 1), 449u);
    if (!full_hash) out[j] %= (uint32_t)t->memory;
  }
  return 0;
}

/* getFeatureLocation (tile_coding.h:116-151) over a caller-held claim table (indices_: `memory` slots, -1 = free): each of the n
 * hash sums walks from h % memory, wrapping at the table's end, past slots claimed by OTHER hash sums, to a free slot or its
 * own; with `claim` it takes the slot (project(in) always, project(base, variants) under safe = 2 only: tile_coding.h:62-73).
 * out may be hash.  Like the reference's, the walk does not end on a table without a free slot. */
void orc_tile_claim(int32_t *table, int memory, const uint32_t *hash, int n, int claim, uint32_t *out)
{
  const uint32_t mem = (uint32_t)memory;
  for (int j = 0; j < n; ++j)
  {
    const uint32_t h = hash[j];
    uint32_t ii = h % mem;
    while (table[ii] != (int32_t)h && table[ii] != -1)
      if (++ii >= mem) ii = 0;
    if (claim) table[ii] = (int32_t)h;
    out[j] = ii;
  }
}
