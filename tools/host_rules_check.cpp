// host_rules_check.cpp -- the host-side rules of the C ABI (grl_amd/csrc/grlx_host_rules.h) checked as a program of their own, built
// with the host sanitizers (tests/test_host_rules.py).  Each rule is held to the property it states, not to a second copy of its code.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include <cstring>
#include "../grl_amd/csrc/grlx_host_rules.h"

using namespace grlx;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

static void check_growth()
{
  long cases = 0;
  for (uint32_t logC = 8; logC <= 26; ++logC)
    for (uint32_t logC_max = logC; logC_max <= 26; ++logC_max)
      for (uint32_t k = 0; k <= 27; ++k)
        for (int d = -1; d <= 1; ++d)
        {
          const uint32_t used = (uint32_t)((1ll << k) + d);
          const uint64_t cap = 1ull << logC;
          const uint32_t w = growth_target(used, logC, logC_max);
          ++cases;
          CHECK(w >= logC && w <= logC_max, "used %u logC %u max %u -> %u is outside [logC, logC_max]", used, logC, logC_max, w);
          if ((uint64_t)used * 4 <= cap)
          {
            CHECK(w == logC, "used %u logC %u max %u -> %u: at most a quarter full, the tables stay", used, logC, logC_max, w);
            continue;
          }
          const bool eighth = (uint64_t)used * 8 <= (1ull << w);
          CHECK(eighth || w == logC_max, "used %u logC %u max %u -> %u: more than an eighth full below the bound", used, logC, logC_max, w);
          // minimal: one size smaller (where there is one) would be more than an eighth full
          if (w > logC) CHECK((uint64_t)used * 8 > (1ull << (w - 1)), "used %u logC %u max %u -> %u is not the smallest size", used, logC, logC_max, w);
        }
  printf("growth_target: %ld cases\n", cases);
}

static void check_draws()
{
  // the sums of grlx_create's seeding: the representation's memory (outputs = 1), plus the second table of the actor-critic and of QV,
  // plus the target network's own initial draws
  const struct { int agent, target_interval; uint64_t want; const char *what; } rows[5] = {
    {GRLX_AGENT_SARSA, 0, 1000, "sarsa"},
    {GRLX_AGENT_Q, 7, 1000 + 1000, "q with a target network"},
    {GRLX_AGENT_AC, 0, 1000 + 300, "actor-critic"},
    {GRLX_AGENT_QV, 0, 1000 + 300, "qv"},
    {GRLX_AGENT_ADVANTAGE, 0, 1000, "advantage"},
  };
  for (const auto &r : rows)
  {
    grlx_config c;
    memset(&c, 0, sizeof(c));
    c.agent = r.agent;
    c.target_interval = r.target_interval;
    c.projector.memory = 1000;
    c.actor_projector.memory = 300;
    CHECK(table_draws(c) == r.want, "%s: %llu draws, %llu expected", r.what, (unsigned long long)table_draws(c), (unsigned long long)r.want);
  }
  // the jump over them is the stream stepped that many times
  uint64_t x = h_seed(7), y = x;
  for (int i = 0; i < 1300; ++i) y = h_next(y);
  CHECK(h_jump(x, 1300) == y, "h_jump(x, 1300) is not 1300 steps of h_next");
  printf("table_draws: 5 combinations\n");
}

static void check_bytes()
{ // the largest context the ABI admits: 2^26 entries per table, 65,536 replicas -- nothing may wrap at 32 bits
  const size_t N = 65536;
  CHECK((unsigned long long)table_bytes(N, 1, 26) == (1ull << 46), "table_bytes(65536, 1, 26) = %llu", (unsigned long long)table_bytes(N, 1, 26));
  CHECK((unsigned long long)table_bytes(N, 2, 26) == (1ull << 47), "table_bytes(65536, 2, 26) = %llu", (unsigned long long)table_bytes(N, 2, 26));
  CHECK((unsigned long long)tval_bytes(N, 26) == (1ull << 45), "tval_bytes(65536, 26) = %llu", (unsigned long long)tval_bytes(N, 26));
  CHECK((unsigned long long)trace_words(N) == 65536ull * 320ull, "trace_words(65536) = %llu", (unsigned long long)trace_words(N));
  CHECK(table_bytes(3, 2, 8) == 3 * 2 * 16 * 256 && tval_bytes(3, 8) == 3 * 8 * 256 && trace_words(3) == 960, "small sizes");
  printf("byte counts: no 32-bit overflow at 2^26 entries x 65536 replicas\n");
}

static void check_quant()
{ // the property the rule is there for: an admitted coordinate's floor(x * scaling) is an int of magnitude at most 2^30, so tile_quant's
  // cast is defined and the displacement 1 + 2 i added over 32 tilings stays inside int; the first product at the bound is refused
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double scalings[5] = {1., 16. / 0.31415, 16. / 2.5, 32. / 0.1, 1. / 1024.};
  long cases = 0;
  for (double sc : scalings)
  {
    double inside = 1073741824. / sc;                   // walk down to the largest x whose product is below 2^30, up to the first at it
    while (!(inside * sc < 1073741824.)) inside = std::nextafter(inside, 0.);
    while (std::nextafter(inside, inf) * sc < 1073741824.) inside = std::nextafter(inside, inf);
    const double outside = std::nextafter(inside, inf);
    for (double sign : {1., -1.})
    {
      ++cases;
      CHECK(quant_admits(sign * inside, sc), "scaling %g: %a is inside the bound", sc, sign * inside);
      CHECK(!quant_admits(sign * outside, sc), "scaling %g: %a is the first value outside the bound", sc, sign * outside);
      const double q = std::floor(sign * inside * sc);
      CHECK(q >= -1073741824. && q < 1073741824. && (double)(int)q == q, "scaling %g: floor(%a * scaling) = %.17g does not fit", sc, sign * inside, q);
    }
    for (double x : {0., -0., 1e-300, -1e-12, 40., -40.}) CHECK(quant_admits(x, sc), "scaling %g: %g is admitted", sc, x);
    for (double x : {inf, -inf, nan, 1e300, -1e300}) CHECK(!quant_admits(x, sc), "scaling %g: %g is refused", sc, x);
  }
  // rows: the first offender is named by row and dimension, and by kind (1 not finite, 2 out of range); clean rows give 0
  const double sc3[3] = {1., 2., 4.};
  double rows[4 * 3] = {0, 1, 2, -3, 4, 5, 6, 7, 8, 9, 10, 11};
  int row = -1, dim = -1;
  CHECK(quant_admit_rows(rows, 4, 3, sc3, &row, &dim) == 0 && row == -1 && dim == -1, "clean rows");
  CHECK(quant_admit_rows(rows, 0, 3, sc3, &row, &dim) == 0, "no rows");
  rows[2 * 3 + 1] = 536870912.;                         // x 2 = 2^30
  rows[3 * 3 + 0] = nan;
  CHECK(quant_admit_rows(rows, 4, 3, sc3, &row, &dim) == 2 && row == 2 && dim == 1, "out of range at (2, 1): got (%d, %d)", row, dim);
  rows[2 * 3 + 1] = std::nextafter(536870912., 0.);
  CHECK(quant_admit_rows(rows, 4, 3, sc3, &row, &dim) == 1 && row == 3 && dim == 0, "not finite at (3, 0): got (%d, %d)", row, dim);
  rows[3 * 3 + 0] = -inf;
  CHECK(quant_admit_rows(rows, 4, 3, sc3, &row, &dim) == 1 && row == 3 && dim == 0, "-inf at (3, 0): got (%d, %d)", row, dim);
  printf("quant_admits: %ld bounds\n", cases);
}

int main()
{
  check_quant();
  check_growth();
  check_draws();
  check_bytes();
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("host rules ok\n");
  return 0;
}
