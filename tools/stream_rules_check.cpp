// stream_rules_check.cpp -- the chunk rule of grlx_evaluate_trajectory_stream (grl_amd/csrc/grlx_host_rules.h: stream_start_bytes,
// stream_chunk) checked as a program of its own, built with the host sanitizers (tests/test_trajectory_stream_host.py): a table of cases
// computed by hand, then the rule's stated properties over a grid.
#include <cstdio>
#include <initializer_list>
#include "../grl_amd/csrc/grlx_host_rules.h"

using namespace grlx;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

// The pendulum's shape of the GPU tests: 5 replicas, 40 steps, R = 11, S = 3.  One start state stages
//   its state                      3 * 8                    =     24
//   per replica: records      40 * 11 * 8                   =   3520
//                ret, disc         2 * 8                    =     16
//                final state       3 * 8                    =     24
//                steps, terminal, ties  3 * 4               =     12      -> 3572 per replica, 17860 for five
//   together                                                =  17884 bytes
static const uint64_t kOne = 17884;

static void check_table()
{
  CHECK(stream_start_bytes(5, 40, 11, 3) == kOne, "one start state stages %llu bytes, 17884 by hand", (unsigned long long)stream_start_bytes(5, 40, 11, 3));
  CHECK(stream_out_bytes(5, 40, 11, 3) == kOne - 24, "... of which %llu come back, 17860 by hand", (unsigned long long)stream_out_bytes(5, 40, 11, 3));
  const struct { uint64_t bound; int rows, max_steps, R, S, n_starts, want; const char *what; } rows[] = {
    // the default bound: half of 256 MiB holds 7504 start states, the call has 7
    {256ull << 20, 5, 40, 11, 3, 7, 7, "one chunk"},
    {256ull << 20, 5, 40, 11, 3, 10000, 7504, "the default bound's half: floor(134217728 / 17884)"},
    // half the bound = two start states exactly
    {4 * kOne, 5, 40, 11, 3, 8, 2, "an exact multiple: 8 start states in 4 chunks of 2"},
    {4 * kOne, 5, 40, 11, 3, 7, 2, "a partial last chunk: 2, 2, 2, 1"},
    {6 * kOne - 1, 5, 40, 11, 3, 7, 2, "half the bound one byte short of three start states (the half is rounded down)"},
    {6 * kOne, 5, 40, 11, 3, 7, 3, "half the bound = three start states"},
    // one column against half the bound
    {2 * kOne, 5, 40, 11, 3, 7, 1, "a column equal to half the bound"},
    {2 * kOne + 1, 5, 40, 11, 3, 7, 1, "an odd bound: the half is rounded down to the column"},
    {2 * kOne - 1, 5, 40, 11, 3, 7, -1, "a column one byte over half the bound"},
    {2 * kOne - 2, 5, 40, 11, 3, 7, -1, "a column one byte over half an even bound"},
    {kOne, 5, 40, 11, 3, 7, -1, "a bound grlx_evaluate_trajectory accepts: the column fits the bound, not its half"},
    // nothing to do
    {256ull << 20, 5, 40, 11, 3, 0, 0, "no start states"},
    {256ull << 20, 0, 40, 11, 3, 7, 7, "no replicas: the states alone"},
    // the grid: 16 pairs per block, 2^31 - 1 blocks.  65536 replicas: floor(16 * 2147483647 / 65536) = 524287 start states
    // (524287 * 65536 / 16 = 2147479552 blocks; one more start state would make it 2^31).  One start state stages 24 + 65536 * 140 bytes.
    {2ull * 9175064ull * 600000ull, 65536, 1, 11, 3, 1000000, 524287, "the 2^31 - 1 blocks of a launch"},
    {2ull * 9175064ull * 524287ull, 65536, 1, 11, 3, 1000000, 524287, "the same count from the bytes"},
    {2ull * 9175064ull * 524286ull, 65536, 1, 11, 3, 1000000, 524286, "one fewer from the bytes"},
  };
  for (const auto &r : rows)
  {
    const int got = stream_chunk(r.bound, r.rows, r.max_steps, r.R, r.S, r.n_starts);
    CHECK(got == r.want, "%s: %d start states per chunk, %d by hand", r.what, got, r.want);
  }
  printf("stream_chunk: %zu hand-computed cases\n", sizeof(rows) / sizeof(rows[0]));
}

// the properties the rule states, over bounds around every multiple of a column
static void check_properties()
{
  long cases = 0;
  const int shapes[4][4] = {{5, 40, 11, 3}, {3, 1, 15, 5}, {1, 100000, 22, 11}, {4096, 100, 11, 3}};
  for (const auto &sh : shapes)
  {
    const uint64_t one = stream_start_bytes(sh[0], sh[1], sh[2], sh[3]);
    for (uint64_t m = 0; m <= 9; ++m)
      for (int d = -2; d <= 2; ++d)
        for (int n : {0, 1, 2, 7, 1000})
        {
          if (m == 0 && d < 0) continue;
          const uint64_t bound = m * one + (uint64_t)d, half = bound / 2;
          const int c = stream_chunk(bound, sh[0], sh[1], sh[2], sh[3], n);
          ++cases;
          if (one > half) { CHECK(c == -1, "bound %llu: a column of %llu bytes over the half is refused", (unsigned long long)bound, (unsigned long long)one); continue; }
          CHECK(c >= 0 && c <= n, "bound %llu, %d start states: chunk %d", (unsigned long long)bound, n, c);
          CHECK((uint64_t)c * one <= half, "bound %llu: a chunk of %d exceeds the half", (unsigned long long)bound, c);
          CHECK(c == n || (uint64_t)(c + 1) * one > half, "bound %llu: a chunk of %d is not the largest that fits", (unsigned long long)bound, c);
          CHECK(n == 0 || c >= 1, "bound %llu: a column fits, yet the chunk is empty", (unsigned long long)bound);
          CHECK(((uint64_t)c * (uint64_t)sh[0] + 15) / 16 <= kRuleMaxBlocks, "bound %llu: more than 2^31 - 1 blocks", (unsigned long long)bound);
        }
  }
  printf("stream_chunk: %ld grid cases\n", cases);
}

int main()
{
  check_table();
  check_properties();
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("stream rules ok\n");
  return 0;
}
