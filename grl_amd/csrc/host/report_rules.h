// report_rules.h -- the rules of the host layer that need neither HIP nor a device: names, row texts, row caps and the statistics of
// the report files.  Every rule has this one home; the object units (objects_*.cpp) call it, tools/host_report_check.cpp holds it to
// literal expected values under the host sanitizers (tests/test_host_rules.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <iomanip>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/grlx.h"

namespace grlx_host {
namespace rules {

// what a task provides and environment/modeled forwards (task.h, modeled.cpp:79-114)
static const char *const kTaskOutputs[8] = {"observation_dims", "observation_min", "observation_max", "action_dims",
                                            "action_min",       "action_max",      "reward_min",      "reward_max"};

// ParameterizedRepresentation {action: save | load} (representation.h:201-263): the file of a representation is
// <base>-<config path with '/' -> '_'>.dat, the base of a clone among several carrying the identity "@i".  The reference-side addon
// (integration/addons/grlx/src/grlx.cpp, where it loads `load_file`) follows the same rule.
inline std::string dat_name(const std::string &base, bool many, int clone, std::string config_path)
{
  for (char &ch : config_path)
    if (ch == '/') ch = '_';
  return base + (many ? "@" + std::to_string(clone) : std::string()) + "-" + config_path + ".dat";
}

// entries of table tb's dense parameter vector: 0 = Q / critic, 1 = actor / V
inline int table_memory(const grlx_config &c, int tb) { return tb == 1 ? c.actor_projector.memory : c.projector.memory; }

// clone i of a process is seeded seed + first_clone + i (`grlxd -g N`: first_clone = rank * replicas, so the seeds count over all ranks)
inline std::vector<int64_t> clone_seeds(int64_t seed, int first_clone, int n)
{
  std::vector<int64_t> seeds((size_t)n);
  for (int i = 0; i < n; ++i) seeds[(size_t)i] = seed + first_clone + i;
  return seeds;
}

// the value of one sweep axis for a clone: the axis' own, or the yaml's where the axis is not swept (the -n plan and <output>-<run>-sweep.txt)
inline double sweep_value(const std::vector<double> &axis, double shared, size_t clone) { return axis.empty() ? shared : axis[clone]; }

// <output>-<run>[@clone]<what>.txt; the identity "@i" marks a clone among several (multi.cpp:52-56), what = "" for the rows or "-sweep", ...
inline std::string output_name(const std::string &output, int run, bool many, int clone, const std::string &what)
{
  return output + "-" + std::to_string(run) + (many ? "@" + std::to_string(clone) : std::string()) + what + ".txt";
}

// the reward column of a row as the rows file holds it; the sweep's simple regret is read back from this text
inline std::string reward_text(double reward, bool legacy)
{
  std::ostringstream col;
  if (legacy) col << reward;
  else col << std::setprecision(3) << std::fixed << reward;
  return col.str();
}

// one row of <output>-<run>.txt: the 3-column layout of the reference's committed golden files (legacy), or online_learning.cpp:243
inline std::string row_text(int64_t trial, int64_t steps, double reward, double episode_time, double wall, bool legacy)
{
  std::ostringstream oss;
  oss << std::setw(15) << trial << std::setw(15) << steps << std::setw(15) << reward_text(reward, legacy);
  if (!legacy)
    oss << std::setprecision(3) << std::fixed << std::setw(15) << episode_time << std::setw(15) << reward / episode_time << std::setw(15) << wall;
  return oss.str();
}

// bin/grllib.py:71-75: the mean of the last len(rows) / 20 rewards, read as the reference's workers read them: from the text of the
// clone's output.  The caller refuses a column of fewer than 20 rows.
inline double simple_regret(const std::vector<std::string> &reward_column)
{
  const size_t n = reward_column.size(), sample = n / 20;
  double sum = 0;
  for (size_t k = n - sample; k < n; ++k) sum += strtod(reward_column[k].c_str(), nullptr);
  return sum / (double)sample;
}

// trials a run can take: with a steps budget alone a trial has at least one learning step, and every learning trial may bring a test trial
inline int trial_cap(int trials, int steps, int test_interval) { return trials > 0 ? trials : steps * (test_interval >= 0 ? 2 : 1) + 1; }
// rows those trials can write: one per test trial (every trial without a test interval), and one to spare
inline int max_rows(int trial_cap, int test_interval) { return (test_interval >= 0 ? trial_cap / (test_interval + 1) : trial_cap) + 1; }
// rows a run with -k reserves at least: room for the rows of its continuation
static const int kSnapshotRows = 4096;
inline int reserved_rows(int max_rows, bool snapshot_save) { return snapshot_save && max_rows < kSnapshotRows ? kSnapshotRows : max_rows; }

// The three statistics are NOT one formula: they round differently and the files are compared bit for bit.

// <output>-<run>-sweep.txt and -returns.txt (bin/grlo:46-48): two passes, every sum left to right, the deviation over n - 1.
// x[k * stride], k < n.
inline void mean_sd_two_pass(const double *x, int n, size_t stride, double *mean, double *sd)
{
  double sum = 0;
  for (int k = 0; k < n; ++k) sum += x[(size_t)k * stride];
  *mean = sum / n;
  double sq = 0;
  for (int k = 0; k < n; ++k)
  {
    const double d = x[(size_t)k * stride] - *mean;
    sq += d * d;
  }
  *sd = std::sqrt(sq / (n - 1));
}

// <output>-<run>-policy.txt: from the sums the device returns (grlx_query_ensemble), (sum x^2 - (sum x)^2 / n) / (n - 1), clamped at 0
inline void mean_sd_from_sums(double sum, double sum_sq, int n, double *mean, double *sd)
{
  *mean = sum / n;
  const double var = (sum_sq - sum * sum / n) / (n - 1);
  *sd = std::sqrt(var > 0 ? var : 0.);
}

// <output>-<run>-mean.txt: population variance from the all-reduced {sum, sum of squares, count} of a row, clamped at 0; no clone, no figure
inline void mean_sd_population(double sum, double sum_sq, double count, double *mean, double *sd)
{
  *mean = count > 0 ? sum / count : 0.;
  const double var = count > 0 ? std::fmax(0., sum_sq / count - *mean * *mean) : 0.;
  *sd = std::sqrt(var);
}

} // namespace rules
} // namespace grlx_host
