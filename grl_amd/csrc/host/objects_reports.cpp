// objects_reports.cpp -- the files experiment/online_learning writes after the trial loop of a run: the rows of every clone, and on
// rank 0 the sweep, policy, returns, ensemble and mean files.  Names, row texts and statistics are report_rules.h's.
#include <cmath>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "objects_impl.h"
#include "multi_gpu.h"

namespace grlx_host {

using OnlineImpl = OnlineLearningExperimentImpl;

// <output>-<run>[@i].txt of every clone; replica 0's rewards are the curve run() returns.  A sweep also takes the "simple regret" of
// every clone (rules::simple_regret) from the reward column as it was written, so the figures can be recomputed from the files.
void OnlineImpl::write_rows(const RunPlan &p, grlx_ctx *ctx, int run, RunRows *rows, std::vector<double> *curve) const
{
  const RunOptions &opt = *p.opt;
  const int n = rows->n = grlx_rows(ctx);
  std::vector<int64_t> trial((size_t)n), stp((size_t)n);
  std::vector<double> reward((size_t)n);
  std::vector<double> episode_time((size_t)n);     // total_time: sum of tau = steps of the trial (discrete_time, modeled.cpp:209-212)
  if (p.sweep && n / 20 == 0)
    throw Exception(path() + ": a sweep's simple regret needs at least 20 rows per run (this run wrote " + std::to_string(n) + ")");
  std::vector<std::string> reward_column((size_t)(p.sweep ? n : 0));
  for (int i = 0; i < opt.replicas; ++i)
  {
    grlx_read_rows(ctx, i, 0, n, trial.data(), stp.data(), reward.data());
    grlx_read_row_times(ctx, i, 0, n, episode_time.data());
    std::ofstream ofs;
    if (!output.empty()) ofs.open(rules::output_name(output, run, p.many, p.first_clone + i, ""));
    for (int k = 0; k < n; ++k)
    {
      const std::string row = rules::row_text(trial[(size_t)k], stp[(size_t)k], reward[(size_t)k], episode_time[(size_t)k], rows->wall, opt.legacy_rows);
      if (ofs.is_open()) ofs << row << std::endl;
      if (i == 0 && opt.rank == 0 && opt.print_rows) std::cout << row << std::endl;
      if (p.sweep) reward_column[(size_t)k] = rules::reward_text(reward[(size_t)k], opt.legacy_rows);
    }
    if (i == 0) *curve = reward;
    if (p.sweep) rows->regret.push_back(rules::simple_regret(reward_column));
  }
}

// <output>-<run>-sweep.txt (bin/grlo:46-48): per point its index, the four values, n, avg, stddev (n - 1), stderr = stddev / sqrt(n)
void OnlineImpl::write_sweep_file(const RunPlan &p, int run, const RunRows &rows) const
{
  const RunOptions &opt = *p.opt;
  if (!p.sweep || opt.rank != 0 || output.empty()) return;
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-sweep"));
  const int R = opt.sweep_repetitions, points = opt.replicas / R;
  const double shared[4] = {p.c.alpha, p.c.gamma, p.c.lambda, p.c.epsilon};
  for (int pt = 0; pt < points; ++pt)
  {
    double avg = 0, stddev = 0;
    rules::mean_sd_two_pass(rows.regret.data() + (size_t)pt * (size_t)R, R, 1, &avg, &stddev);
    char line[384];
    int at = snprintf(line, sizeof(line), "%d", pt);
    for (int k = 0; k < 4; ++k)
      at += snprintf(line + at, sizeof(line) - (size_t)at, " %.17g", rules::sweep_value(opt.sweep[k], shared[k], (size_t)pt * (size_t)R));
    snprintf(line + at, sizeof(line) - (size_t)at, " %d %.17g %.17g %.17g", R, avg, stddev, stddev / std::sqrt((double)R));
    ofs << line << std::endl;
  }
}

// -Q, <output>-<run>-policy.txt: the policy after the last trial of the run, grlx_query_ensemble over the clones of every group
void OnlineImpl::write_policy_file(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  const RunOptions &opt = *p.opt;
  if (!p.query || opt.rank != 0) return;
  const int G = p.group, groups = opt.replicas / G, A = p.c.action_steps, cols = 2 + 2 * A;
  std::vector<double> ens((size_t)groups * (size_t)opt.query_rows * (size_t)cols);
  check(grlx_query_ensemble(ctx, 0, opt.replicas, G, opt.query_obs.data(), opt.query_rows, ens.data()), "-Q " + opt.query_file + ": ");
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-policy"));
  double delta = (p.c.action_max - p.c.action_min) / ((double)A - 1);     // UniformDiscretizer::configure (uniform.cpp:60-95)
  if (std::isnan(delta)) delta = 0.;
  for (int g = 0; g < groups; ++g)
    for (int o = 0; o < opt.query_rows; ++o)
    {
      const double *e = ens.data() + ((size_t)g * (size_t)opt.query_rows + (size_t)o) * (size_t)cols;
      double mean = 0, sd = 0;
      rules::mean_sd_from_sums(e[0], e[1], G, &mean, &sd);
      int majority = 0;                                               // the lowest index wins a tie
      for (int a = 1; a < A; ++a)
        if (e[2 + A + a] > e[2 + A + majority]) majority = a;
      if (p.sweep) ofs << std::setw(15) << g;
      for (int i = 0; i < opt.query_cols; ++i) ofs << std::setw(15) << opt.query_obs[(size_t)o * (size_t)opt.query_cols + (size_t)i];
      ofs << std::setw(15) << mean << std::setw(15) << sd;
      for (int a = 0; a < A; ++a) ofs << std::setw(15) << (long long)e[2 + A + a];
      ofs << std::setw(15) << p.c.action_min + delta * majority << std::endl;
    }
}

// -E, <output>-<run>-returns.txt: greedy episodes from the start states of the file, after the last trial of the run; the statistics
// on the host, ascending clones
void OnlineImpl::write_returns_file(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  const RunOptions &opt = *p.opt;
  if (!p.evaluate || opt.rank != 0) return;
  const int G = p.group, groups = opt.replicas / G, NS = opt.evaluate_rows;
  const size_t pairs = (size_t)opt.replicas * (size_t)NS;
  std::vector<double> ret(pairs);
  std::vector<int32_t> esteps(pairs), eterm(pairs), eties(pairs);
  check(grlx_evaluate(ctx, 0, opt.replicas, opt.evaluate_states.data(), NS, 0, ret.data(), nullptr, esteps.data(), eterm.data(), eties.data(), nullptr),
        "-E " + opt.evaluate_file + ": ");
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-returns"));
  for (int g = 0; g < groups; ++g)
    for (int s = 0; s < NS; ++s)
    {
      const size_t first = (size_t)g * (size_t)G * (size_t)NS + (size_t)s;      // clone k of the group: first + k * NS
      double step_sum = 0;
      long long codes[4] = {0, 0, 0, 0}, tie_sum = 0;
      for (int k = 0; k < G; ++k)
      {
        const size_t at = first + (size_t)k * (size_t)NS;
        step_sum += (double)esteps[at];
        codes[eterm[at] & 3]++;
        tie_sum += eties[at];
      }
      double mean = 0, sd = 0;
      rules::mean_sd_two_pass(ret.data() + first, G, (size_t)NS, &mean, &sd);
      char line[384];
      int at = p.sweep ? snprintf(line, sizeof(line), "%d ", g) : 0;
      snprintf(line + at, sizeof(line) - (size_t)at, "%.17g %.17g %.17g %lld %lld %lld %lld %lld", mean, sd, step_sum / G, codes[0], codes[1], codes[2],
               codes[3], tie_sum);
      ofs << line << std::endl;
    }
}

// -E -V, <output>-<run>-ensemble.txt: the same start states on the vote or the mean Q of each group: one episode per (group, start state)
void OnlineImpl::write_ensemble_file(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  const RunOptions &opt = *p.opt;
  if (!p.evaluate || opt.rank != 0 || opt.ensemble_rule < 0) return;
  const int G = p.group, groups = opt.replicas / G, NS = opt.evaluate_rows;
  const size_t gp = (size_t)groups * (size_t)NS;
  std::vector<double> vret(gp), vdisc(gp);
  std::vector<int32_t> vsteps(gp), vterm(gp), vties(gp);
  std::vector<int64_t> vmt(gp), vag(gp);
  check(grlx_evaluate_ensemble(ctx, 0, opt.replicas, G, opt.ensemble_rule, opt.evaluate_states.data(), NS, 0, vret.data(), vdisc.data(), vsteps.data(),
                               vterm.data(), vties.data(), vmt.data(), vag.data(), nullptr),
        "-V: ");
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-ensemble"));
  for (int g = 0; g < groups; ++g)
    for (int s = 0; s < NS; ++s)
    {
      const size_t at = (size_t)g * (size_t)NS + (size_t)s;
      char line[384];
      int n0 = p.sweep ? snprintf(line, sizeof(line), "%d ", g) : 0;
      snprintf(line + n0, sizeof(line) - (size_t)n0, "%.17g %.17g %d %d %d %lld %.17g", vret[at], vdisc[at], vsteps[at], vterm[at], vties[at],
               (long long)vmt[at], (double)vag[at] / ((double)vsteps[at] * (double)G));
      ofs << line << std::endl;
    }
}

// one line per step taken of records[rows][NS][max_steps][R]: "row start step" and the record, the three integer words as integers
static void write_record_lines(std::ofstream &ofs, const std::vector<double> &records, const std::vector<int32_t> &steps, int rows, int NS, int max_steps, int R)
{
  std::string line;
  char word[48];
  for (int k = 0; k < rows; ++k)
    for (int s = 0; s < NS; ++s)
    {
      const size_t pair = (size_t)k * (size_t)NS + (size_t)s;
      for (int t = 0; t < steps[pair]; ++t)
      {
        const double *rec = records.data() + (pair * (size_t)max_steps + (size_t)t) * (size_t)R;
        snprintf(word, sizeof(word), "%d %d %d", k, s, t);
        line = word;
        for (int w = 0; w < R; ++w)
        {
          if (w == GRLX_TRAJ_ACTION_INDEX || w == GRLX_TRAJ_N_MAX || w == GRLX_TRAJ_TERMINAL) snprintf(word, sizeof(word), " %lld", (long long)rec[w]);
          else snprintf(word, sizeof(word), " %.17g", rec[w]);
          line += word;
        }
        ofs << line << '\n';
      }
    }
  ofs.flush();
}

// -E -T, <output>-<run>-trajectories.txt: the first -T steps of the returns file's episodes, step by step; with -V also
// <output>-<run>-ensemble-trajectories.txt, the ensemble file's
void OnlineImpl::write_trajectory_files(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  const RunOptions &opt = *p.opt;
  if (!p.evaluate || opt.rank != 0 || opt.trajectory_steps < 1) return;
  const int G = p.group, groups = opt.replicas / G, NS = opt.evaluate_rows, T = opt.trajectory_steps;
  {
    const int R = grlx_trajectory_record_words(ctx, 0);
    check(R < 0 ? R : GRLX_OK, "-T: ");
    std::vector<double> records((size_t)opt.replicas * (size_t)NS * (size_t)T * (size_t)R);
    std::vector<int32_t> tsteps((size_t)opt.replicas * (size_t)NS);
    check(grlx_evaluate_trajectory(ctx, 0, opt.replicas, opt.evaluate_states.data(), NS, T, nullptr, nullptr, tsteps.data(), nullptr, nullptr, nullptr,
                                   records.data()),
          "-T " + std::to_string(T) + ": ");
    std::ofstream ofs(rules::output_name(output, run, false, 0, "-trajectories"));
    write_record_lines(ofs, records, tsteps, opt.replicas, NS, T, R);
  }
  if (opt.ensemble_rule < 0) return;
  const int R = grlx_trajectory_record_words(ctx, 1);
  check(R < 0 ? R : GRLX_OK, "-T -V: ");
  std::vector<double> records((size_t)groups * (size_t)NS * (size_t)T * (size_t)R);
  std::vector<int32_t> tsteps((size_t)groups * (size_t)NS);
  check(grlx_evaluate_ensemble_trajectory(ctx, 0, opt.replicas, G, opt.ensemble_rule, opt.evaluate_states.data(), NS, T, nullptr, nullptr, tsteps.data(),
                                          nullptr, nullptr, nullptr, nullptr, nullptr, records.data()),
        "-T " + std::to_string(T) + " -V: ");
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-ensemble-trajectories"));
  write_record_lines(ofs, records, tsteps, groups, NS, T, R);
}

// -E -e, <output>-<run>-sampled.txt: the returns file's start states under a sampler (grlx_evaluate_sampled) on the streams of
// grlx_episode_streams(-s seed): the returns file's columns and the summed explored steps; the statistics on the host, ascending clones.
// With -T also <output>-<run>-sampled-trajectories.txt, the first -T steps of sampled episodes on the same streams, step by step.
void OnlineImpl::write_sampled_files(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  const RunOptions &opt = *p.opt;
  if (!p.evaluate || opt.rank != 0 || opt.sampled_sampler < 0) return;
  const int G = p.group, groups = opt.replicas / G, NS = opt.evaluate_rows;
  const size_t pairs = (size_t)opt.replicas * (size_t)NS;
  std::vector<uint64_t> streams(pairs * 2);
  grlx_episode_streams(opt.seed, 0, (int64_t)pairs, streams.data());
  std::vector<double> ret(pairs);
  std::vector<int32_t> esteps(pairs), eterm(pairs), eties(pairs), eexp(pairs);
  check(grlx_evaluate_sampled(ctx, 0, opt.replicas, opt.evaluate_states.data(), NS, 0, opt.sampled_sampler, opt.sampled_epsilon, streams.data(), ret.data(),
                              nullptr, esteps.data(), eterm.data(), eties.data(), eexp.data(), nullptr, nullptr),
        "-e " + opt.sampled_arg + ": ");
  {
    std::ofstream ofs(rules::output_name(output, run, false, 0, "-sampled"));
    for (int g = 0; g < groups; ++g)
      for (int s = 0; s < NS; ++s)
      {
        const size_t first = (size_t)g * (size_t)G * (size_t)NS + (size_t)s;      // clone k of the group: first + k * NS
        double step_sum = 0;
        long long codes[4] = {0, 0, 0, 0}, tie_sum = 0, explored_sum = 0;
        for (int k = 0; k < G; ++k)
        {
          const size_t at = first + (size_t)k * (size_t)NS;
          step_sum += (double)esteps[at];
          codes[eterm[at] & 3]++;
          tie_sum += eties[at];
          explored_sum += eexp[at];
        }
        double mean = 0, sd = 0;
        rules::mean_sd_two_pass(ret.data() + first, G, (size_t)NS, &mean, &sd);
        char line[416];
        int at = p.sweep ? snprintf(line, sizeof(line), "%d ", g) : 0;
        snprintf(line + at, sizeof(line) - (size_t)at, "%.17g %.17g %.17g %lld %lld %lld %lld %lld %lld", mean, sd, step_sum / G, codes[0], codes[1], codes[2],
                 codes[3], tie_sum, explored_sum);
        ofs << line << std::endl;
      }
  }
  if (opt.trajectory_steps < 1) return;
  const int T = opt.trajectory_steps, R = grlx_sampled_trajectory_record_words(ctx);
  check(R < 0 ? R : GRLX_OK, "-e -T: ");
  std::vector<double> records(pairs * (size_t)T * (size_t)R);
  std::vector<int32_t> tsteps(pairs);
  check(grlx_evaluate_sampled_trajectory(ctx, 0, opt.replicas, opt.evaluate_states.data(), NS, T, opt.sampled_sampler, opt.sampled_epsilon, streams.data(),
                                         nullptr, nullptr, tsteps.data(), nullptr, nullptr, nullptr, nullptr, nullptr, records.data()),
        "-e " + opt.sampled_arg + " -T " + std::to_string(T) + ": ");
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-sampled-trajectories"));
  write_record_lines(ofs, records, tsteps, opt.replicas, NS, T, R);
}

// -E -N, <output>-<run>-noisy.txt: the returns file's start states of an actor-critic under its exploring policy (grlx_evaluate_noisy) on the
// configuration's theta, the streams of grlx_episode_stream_words(-s seed) and a noise state of 0: the returns file's columns (ties: 0) and
// the summed clipped steps; the statistics on the host, ascending clones.  With -T also <output>-<run>-noisy-trajectories.txt, the first
// -T steps of noisy episodes on the same streams, step by step.
void OnlineImpl::write_noisy_files(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  const RunOptions &opt = *p.opt;
  if (!p.evaluate || opt.rank != 0 || !opt.noisy) return;
  const int G = p.group, groups = opt.replicas / G, NS = opt.evaluate_rows;
  const size_t pairs = (size_t)opt.replicas * (size_t)NS;
  std::vector<uint64_t> streams(pairs);
  grlx_episode_stream_words(opt.seed, 0, (int64_t)pairs, streams.data());
  std::vector<double> ret(pairs);
  std::vector<int32_t> esteps(pairs), eterm(pairs), eclip(pairs);
  check(grlx_evaluate_noisy(ctx, 0, opt.replicas, opt.evaluate_states.data(), NS, 0, opt.noisy_sigma, GRLX_THETA_OWN, streams.data(), nullptr, ret.data(),
                            nullptr, esteps.data(), eterm.data(), eclip.data(), nullptr, nullptr, nullptr),
        "-N " + opt.noisy_arg + ": ");
  {
    std::ofstream ofs(rules::output_name(output, run, false, 0, "-noisy"));
    for (int g = 0; g < groups; ++g)
      for (int s = 0; s < NS; ++s)
      {
        const size_t first = (size_t)g * (size_t)G * (size_t)NS + (size_t)s;      // clone k of the group: first + k * NS
        double step_sum = 0;
        long long codes[4] = {0, 0, 0, 0}, clipped_sum = 0;
        for (int k = 0; k < G; ++k)
        {
          const size_t at = first + (size_t)k * (size_t)NS;
          step_sum += (double)esteps[at];
          codes[eterm[at] & 3]++;
          clipped_sum += eclip[at];
        }
        double mean = 0, sd = 0;
        rules::mean_sd_two_pass(ret.data() + first, G, (size_t)NS, &mean, &sd);
        char line[416];
        snprintf(line, sizeof(line), "%.17g %.17g %.17g %lld %lld %lld %lld %lld %lld", mean, sd, step_sum / G, codes[0], codes[1], codes[2], codes[3], 0ll,
                 clipped_sum);
        ofs << line << std::endl;
      }
  }
  if (opt.trajectory_steps < 1) return;
  const int T = opt.trajectory_steps, R = grlx_noisy_trajectory_record_words(ctx);
  check(R < 0 ? R : GRLX_OK, "-N -T: ");
  std::vector<double> records(pairs * (size_t)T * (size_t)R);
  std::vector<int32_t> tsteps(pairs);
  check(grlx_evaluate_noisy_trajectory(ctx, 0, opt.replicas, opt.evaluate_states.data(), NS, T, opt.noisy_sigma, GRLX_THETA_OWN, streams.data(), nullptr,
                                       nullptr, nullptr, tsteps.data(), nullptr, nullptr, nullptr, nullptr, nullptr, records.data()),
        "-N " + opt.noisy_arg + " -T " + std::to_string(T) + ": ");
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-noisy-trajectories"));
  write_record_lines(ofs, records, tsteps, opt.replicas, NS, T, R);
}

// -E -A, <output>-<run>-actor-ensemble.txt: the returns file's start states for the ensemble of ALL clones of an actor-critic on the members'
// combined action (grlx_evaluate_actor_ensemble), one line per start state: ret disc steps terminal ties kept spread.  With -T also
// <output>-<run>-actor-ensemble-trajectories.txt, the first -T steps of the same episodes, step by step, as group 0's lines.
void OnlineImpl::write_actor_ensemble_files(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  const RunOptions &opt = *p.opt;
  if (!p.evaluate || opt.rank != 0 || opt.actor_rule < 0) return;
  const int NS = opt.evaluate_rows, G = opt.replicas;
  std::vector<double> ret((size_t)NS), disc((size_t)NS), spread((size_t)NS);
  std::vector<int32_t> esteps((size_t)NS), eterm((size_t)NS), eties((size_t)NS);
  std::vector<int64_t> kept((size_t)NS);
  check(grlx_evaluate_actor_ensemble(ctx, 0, G, G, opt.actor_rule, opt.actor_bins, opt.actor_r, opt.evaluate_states.data(), NS, 0, ret.data(), disc.data(),
                                     esteps.data(), eterm.data(), eties.data(), kept.data(), spread.data(), nullptr),
        "-A " + opt.actor_arg + ": ");
  {
    std::ofstream ofs(rules::output_name(output, run, false, 0, "-actor-ensemble"));
    for (int s = 0; s < NS; ++s)
    {
      char line[416];
      snprintf(line, sizeof(line), "%.17g %.17g %d %d %d %lld %.17g", ret[s], disc[s], esteps[s], eterm[s], eties[s], (long long)kept[s], spread[s]);
      ofs << line << std::endl;
    }
  }
  if (opt.trajectory_steps < 1) return;
  const int T = opt.trajectory_steps, R = grlx_actor_ensemble_trajectory_record_words(ctx);
  check(R < 0 ? R : GRLX_OK, "-A -T: ");
  std::vector<double> records((size_t)NS * (size_t)T * (size_t)R);
  std::vector<int32_t> tsteps((size_t)NS);
  check(grlx_evaluate_actor_ensemble_trajectory(ctx, 0, G, G, opt.actor_rule, opt.actor_bins, opt.actor_r, opt.evaluate_states.data(), NS, T, nullptr, nullptr,
                                                tsteps.data(), nullptr, nullptr, nullptr, nullptr, nullptr, records.data()),
        "-A " + opt.actor_arg + " -T " + std::to_string(T) + ": ");
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-actor-ensemble-trajectories"));
  write_record_lines(ofs, records, tsteps, 1, NS, T, R);
}

// `grlxd -g N`, <output>-<run>-mean.txt: the learning curve over the clones of ALL ranks: per row {sum, sum of squares, count} of this
// device's replicas (grlx_curve_stats, fixed reduction order), ONE all-reduce over the ranks, mean and standard deviation on rank 0.
// (Trial-bounded runs write the same rows on every rank; a steps budget with more than one clone is refused by the plan.)
void OnlineImpl::write_mean_file(const RunPlan &p, grlx_ctx *ctx, int run, const RunRows &rows) const
{
  const RunOptions &opt = *p.opt;
  const int n = rows.n;
  if (!opt.reducer || n <= 0) return;
  double *dev = opt.reducer->device_buffer((size_t)n * 3);
  check(grlx_curve_stats(ctx, 0, n, dev, nullptr));
  check(grlx_sync(ctx, nullptr));
  opt.reducer->all_reduce_sum(dev, (size_t)n * 3);
  std::vector<double> st((size_t)n * 3);
  opt.reducer->to_host(st.data(), dev, st.size());
  if (opt.rank != 0 || output.empty()) return;
  std::ofstream ofs(rules::output_name(output, run, false, 0, "-mean"));
  std::vector<int64_t> trial((size_t)n), stp((size_t)n);
  std::vector<double> reward((size_t)n);
  grlx_read_rows(ctx, 0, 0, n, trial.data(), stp.data(), reward.data());
  for (int k = 0; k < n; ++k)
  { // trial, clones that wrote the row, mean return, standard deviation over the clones (population)
    const double cntk = st[(size_t)k * 3 + 2];
    double mean = 0, sd = 0;
    rules::mean_sd_population(st[(size_t)k * 3], st[(size_t)k * 3 + 1], cntk, &mean, &sd);
    ofs << std::setw(15) << trial[(size_t)k] << std::setw(15) << (long long)cntk << std::setw(20) << std::setprecision(12) << mean
        << std::setw(20) << std::setprecision(12) << sd << std::endl;
  }
}

} // namespace grlx_host
