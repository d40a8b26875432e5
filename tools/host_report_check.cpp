// host_report_check.cpp -- the device-free rules of the host layer (grl_amd/csrc/host/report_rules.h) checked as a program of their
// own, built with the host sanitizers (tests/test_host_rules.py).  Names and row texts are held to literal strings -- the rows are the
// first and the last of tests/golden/pendulum-sarsa-tc-0.txt --, the caps and statistics to values worked out by hand.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "../grl_amd/csrc/host/report_rules.h"

using namespace grlx_host::rules;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)
#define CHECK_STR(got, want) CHECK((got) == std::string(want), "'%s', expected '%s'", (got).c_str(), want)

static void check_names()
{
  CHECK_STR(output_name("out", 0, false, 0, ""), "out-0.txt");                       // one clone: no identity
  CHECK_STR(output_name("out", 1, true, 3, ""), "out-1@3.txt");                      // many clones
  CHECK_STR(output_name("out", 0, true, 2 * 4 + 1, ""), "out-0@9.txt");              // rank 2 of a job with 4 clones per rank, its clone 1
  CHECK_STR(output_name("dir/out", 2, false, 0, "-sweep"), "dir/out-2-sweep.txt");
  CHECK_STR(dat_name("out-run0", false, 0, "experiment/agent/policy/representation"), "out-run0-experiment_agent_policy_representation.dat");
  CHECK_STR(dat_name("out-run0-trial10", true, 2, "experiment/agent/predictor/critic/representation"),
            "out-run0-trial10@2-experiment_agent_predictor_critic_representation.dat");
  const std::vector<int64_t> seeds = clone_seeds(5, 2 * 4, 3);
  CHECK(seeds.size() == 3 && seeds[0] == 13 && seeds[1] == 14 && seeds[2] == 15, "clone_seeds(5, 8, 3)");
  CHECK(clone_seeds(1, 0, 0).empty(), "no clones, no seeds");
  const std::vector<double> axis = {0.1, 0.2, 0.3}, none;
  CHECK(sweep_value(axis, 0.5, 2) == 0.3 && sweep_value(none, 0.5, 2) == 0.5, "sweep_value");
  grlx_config c;
  memset(&c, 0, sizeof(c));
  c.projector.memory = 1000;
  c.actor_projector.memory = 300;
  CHECK(table_memory(c, 0) == 1000 && table_memory(c, 1) == 300, "table_memory");
  CHECK(sizeof(kTaskOutputs) / sizeof(kTaskOutputs[0]) == 8 && !strcmp(kTaskOutputs[0], "observation_dims") && !strcmp(kTaskOutputs[7], "reward_max"),
        "the eight task outputs");
  printf("names: ok\n");
}

static void check_rows()
{
  // the 3-column layout, against the golden file's first and last row
  CHECK_STR(row_text(10, 1000, -4935.85, 99, 1.25, true), "             10           1000       -4935.85");
  CHECK_STR(row_text(1810, 181000, -907.596, 100, 1.25, true), "           1810         181000       -907.596");
  // the same rows in the six-column layout: reward, episode time, reward per time and wall time with three decimals
  CHECK_STR(row_text(10, 1000, -4935.85, 99, 1.25, false), "             10           1000      -4935.850         99.000        -49.857          1.250");
  CHECK_STR(row_text(1810, 181000, -907.596, 100, 1.25, false), "           1810         181000       -907.596        100.000         -9.076          1.250");
  CHECK_STR(reward_text(-4935.85, true), "-4935.85");
  CHECK_STR(reward_text(-4935.85, false), "-4935.850");
  CHECK_STR(reward_text(1.23456, false), "1.235");                                  // the text is not the value
  printf("rows: ok\n");
}

static void check_regret()
{ // 40 rows: the sample is the last two.  Their values are 1.23456 and -2.0004; their %.3f texts 1.235 and -2.000.
  std::vector<std::string> fixed, plain;
  for (int k = 0; k < 40; ++k)
  {
    const double r = k == 38 ? 1.23456 : k == 39 ? -2.0004 : -1000. - k;
    fixed.push_back(reward_text(r, false));
    plain.push_back(reward_text(r, true));
  }
  const double got = simple_regret(fixed);
  CHECK(got == (1.235 + -2.000) / 2 && std::fabs(got - -0.3825) < 1e-15, "regret of the %%.3f column: %.17g, expected -0.3825", got);
  CHECK(got != (1.23456 + -2.0004) / 2, "the regret is read from the text, not from the values");
  const double got_plain = simple_regret(plain);
  CHECK(got_plain == (1.23456 + -2.0004) / 2, "regret of the 3-column layout: %.17g", got_plain);
  // 59 rows: still a sample of two; 60: three
  std::vector<std::string> col(59, "1");
  col[56] = "100";
  CHECK(simple_regret(col) == 1., "59 rows: %.17g", simple_regret(col));
  col.push_back("1");
  col[57] = "4";
  CHECK(simple_regret(col) == 2., "60 rows: %.17g", simple_regret(col));
  printf("regret: ok\n");
}

static void check_caps()
{
  // trials only: every trial a row, or one row per test trial
  CHECK(trial_cap(100, 0, -1) == 100 && max_rows(100, -1) == 101, "trials only, no test interval");
  CHECK(trial_cap(100, 0, 10) == 100 && max_rows(100, 10) == 100 / 11 + 1, "trials only, test interval 10");
  CHECK(trial_cap(100, 2450, 10) == 100, "trials bound the run where both are given");
  // steps only: a trial has at least one learning step; with a test interval a test trial may follow every learning trial
  CHECK(trial_cap(0, 2450, -1) == 2451 && max_rows(2451, -1) == 2452, "steps only, no test interval");
  CHECK(trial_cap(0, 2450, 10) == 4901 && max_rows(4901, 10) == 446, "steps only, test interval 10: %d", max_rows(trial_cap(0, 2450, 10), 10));
  // -k: at least kSnapshotRows
  CHECK(kSnapshotRows == 4096 && reserved_rows(10, true) == 4096 && reserved_rows(10, false) == 10 && reserved_rows(5000, true) == 5000, "the -k floor");
  printf("row caps: ok\n");
}

static void check_statistics()
{
  double mean = -1, sd = -1;
  const double x[5] = {1, 9, 2, 9, 3};
  mean_sd_two_pass(x, 3, 2, &mean, &sd);                                            // 1, 2, 3: mean 2, deviation over n - 1 exactly 1
  CHECK(mean == 2. && sd == 1., "two-pass over a stride: %.17g %.17g", mean, sd);
  const double y[3] = {1, 2, 4};                                                    // mean 7/3, sum of squared deviations 42/9, over 2: 7/3
  mean_sd_two_pass(y, 3, 1, &mean, &sd);
  CHECK(mean == 7. / 3 && std::fabs(sd - std::sqrt(7. / 3)) < 1e-15, "two-pass: %.17g %.17g", mean, sd);
  mean_sd_from_sums(6, 14, 3, &mean, &sd);                                          // the same 1, 2, 3 from their sums: (14 - 36 / 3) / 2 = 1
  CHECK(mean == 2. && sd == 1., "from sums: %.17g %.17g", mean, sd);
  mean_sd_from_sums(3, 2.9999999, 3, &mean, &sd);                                   // rounding below zero is clamped, not a NaN
  CHECK(mean == 1. && sd == 0., "from sums, clamped: %.17g %.17g", mean, sd);
  mean_sd_population(6, 14, 3, &mean, &sd);                                         // population: 14 / 3 - 4 = 2 / 3
  CHECK(mean == 2. && std::fabs(sd - std::sqrt(2. / 3)) < 1e-12, "population: %.17g %.17g", mean, sd);
  const double s = 0.1 + 0.1 + 0.1, q = 0.1 * 0.1 + 0.1 * 0.1 + 0.1 * 0.1;          // a constant column: whatever the rounding, no NaN
  mean_sd_population(s, q, 3, &mean, &sd);
  CHECK(std::fabs(mean - 0.1) < 1e-15 && sd >= 0 && sd < 1e-7, "population, constant column: %.17g %.17g", mean, sd);
  mean_sd_population(3, 2.9999999, 3, &mean, &sd);
  CHECK(mean == 1. && sd == 0., "population, clamped: %.17g %.17g", mean, sd);
  mean_sd_population(0, 0, 0, &mean, &sd);                                          // a row no clone wrote
  CHECK(mean == 0. && sd == 0., "population, no clone: %.17g %.17g", mean, sd);
  printf("statistics: ok\n");
}

int main()
{
  check_names();
  check_rows();
  check_regret();
  check_caps();
  check_statistics();
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("host report rules ok\n");
  return 0;
}
