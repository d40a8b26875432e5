// grlxd.cpp -- deployer for the accelerated path, command-line compatible with the
// reference's `grld [-v] [-s seed] <yaml file> [yaml file...]` (base/src/deployer.cpp:38-150),
// plus -r replicas, -t trials (override), -l (3-column golden layout), -q (no rows on stdout),
// -p <path>=v1,v2,... (repeatable): a grid sweep over predictor alpha / gamma / lambda and the sampler's epsilon, the study of the reference's
// bin/grlo as the clones of one run: -r is then the repetitions per point, clone i = point * repetitions + k (points: the Cartesian product
// in the order of the -p options, the last fastest) with seed + i and identity "@i"; <output>-<run>-sweep.txt holds the statistics per point,
// -k FILE: write a snapshot of the whole context (grlx_snapshot_save) when the trial loop of the run ends; -K FILE: start from one and continue
// its trial loop up to trials: / -t -- the output files are those of the uninterrupted run, byte for byte,
// -Q FILE: after the last trial of every run, query the policy at the observations of FILE (one per line) over the clones and write
// <output>-<run>-policy.txt: observation, mean and standard deviation (n - 1) of the value, votes per action, the majority action (objects.h),
// -E FILE: after the last trial of every run, one greedy episode per (clone, start state) from the model states of FILE (one per line) with
// grlx_evaluate, and <output>-<run>-returns.txt: mean and standard deviation (n - 1) of the return, mean steps, the count of every terminal
// code and the summed ties over the clones (objects.h),
// -V vote|mean: with -E, also one episode per start state of the ensemble of all clones (with -p: of each point's repetitions) acting on
// the members' vote or on their mean Q (grlx_evaluate_ensemble), written to <output>-<run>-ensemble.txt (objects.h),
// -T STEPS: with -E, also the steps of those episodes, STEPS of each at the most (grlx_evaluate_trajectory), one line per step taken in
// <output>-<run>-trajectories.txt, and with -V the ensemble's in <output>-<run>-ensemble-trajectories.txt (objects.h),
// -e EPSILON|own|greedy: with -E, also one SAMPLED episode per (clone, start state) with grlx_evaluate_sampled -- the epsilon-greedy sampler on
// EPSILON in [0, 1] or on every clone's own decayed epsilon, or the greedy sampler with its drawn tie break -- on the streams of
// grlx_episode_streams(-s seed), written to <output>-<run>-sampled.txt, and with -T the steps in <output>-<run>-sampled-trajectories.txt (objects.h),
// -N SIGMA|own: with -E on an actor-critic, also one NOISY episode per (clone, start state) with grlx_evaluate_noisy -- the exploring policy on a
// standard deviation SIGMA >= 0 or on every clone's own decayed sigma, on the configuration's theta -- on the streams of
// grlx_episode_stream_words(-s seed), written to <output>-<run>-noisy.txt, and with -T the steps in <output>-<run>-noisy-trajectories.txt (objects.h),
// -A mean|binning[:bins]|data_center[:keep]|density[:r]: with -E on an actor-critic, also one episode per start state of the ensemble of ALL clones
// acting on the members' combined action (grlx_evaluate_actor_ensemble; the parameters default to the reference's 10, 10 and 0.001), written to
// <output>-<run>-actor-ensemble.txt, and with -T the steps in <output>-<run>-actor-ensemble-trajectories.txt (objects.h),
// -n: print the plan (one line per clone: i seed alpha gamma lambda epsilon) and exit before anything touches HIP, and
// -g N: one process per GPU (rank r on the r-th visible device, started before anything touches HIP), every rank running -r replicas
// (clones r * replicas ..., seeds and "@i" identities counted over the whole job), the learning curves reduced with one RCCL all-reduce
// per run (multi_gpu.h); rank 0 prints the rows and writes <output>-<run>-mean.txt.  The model is experiment/multi (multi.cpp:44-75).
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <vector>

#include "../../../include/grlx.h"
#include "configurable.h"
#include "multi_gpu.h"
#include "objects.h"

using namespace grlx_host;

namespace {
// the parameters a sweep may vary: the four of the reference's bin/optimize.yaml that the device path holds per replica (index: GRLX_PARAM_*)
const char *const kSweepPaths[4] = {"/experiment/agent/predictor/alpha", "/experiment/agent/predictor/gamma", "/experiment/agent/predictor/lambda",
                                    "/experiment/agent/policy/sampler/epsilon"};
struct SweepAxis { int param; std::vector<double> values; };

SweepAxis parse_sweep_axis(const std::string &arg)
{
  const size_t eq = arg.find('=');
  const std::string path = arg.substr(0, eq);
  SweepAxis axis;
  axis.param = -1;
  for (int k = 0; k < 4; ++k)
    if (path == kSweepPaths[k]) axis.param = k;
  if (axis.param < 0)
    throw Exception("-p: unknown path '" + path + "' (a sweep varies " + kSweepPaths[0] + ", " + kSweepPaths[1] + ", " + kSweepPaths[2] + " or " + kSweepPaths[3] + ")");
  const std::string list = eq == std::string::npos ? "" : arg.substr(eq + 1);
  for (size_t at = 0; at < list.size();)
  {
    size_t end = list.find(',', at);
    if (end == std::string::npos) end = list.size();
    const std::string item = list.substr(at, end - at);
    char *stop = nullptr;
    const double v = strtod(item.c_str(), &stop);
    if (item.empty() || *stop != 0) throw Exception("-p " + path + ": '" + item + "' is not a number");
    axis.values.push_back(v);
    at = end + 1;
  }
  if (axis.values.empty() || (!list.empty() && list.back() == ',')) throw Exception("-p " + path + ": empty value list (expected " + path + "=v1,v2,...)");
  return axis;
}
} // namespace

int main(int argc, char **argv)
{
  RunOptions opt;
  int trials_override = -1;
  int gpus = 0;
  int c;
  std::vector<std::string> sweep_args;
  std::string ensemble_arg;
  bool ensemble = false, trajectory = false, sampled = false, noisy = false, actors = false;
  int trajectory_steps = 0;
  while ((c = getopt(argc, argv, "vs:r:t:lqc:g:p:nk:K:Q:E:V:T:e:N:A:")) != -1)
  {
    switch (c)
    {
      case 'v': log_verbosity++; break;
      case 's': opt.seed = atol(optarg); break;
      case 'r': opt.replicas = atoi(optarg); break;
      case 't': trials_override = atoi(optarg); break;
      case 'l': opt.legacy_rows = true; break;
      case 'q': opt.print_rows = false; break;
      case 'c': opt.table_log2_capacity = atoi(optarg); break;
      case 'g': gpus = atoi(optarg); break;
      case 'p': sweep_args.push_back(optarg); break;
      case 'n': opt.plan_only = true; break;
      case 'k': opt.snapshot_save = optarg; break;
      case 'K': opt.snapshot_load = optarg; break;
      case 'Q': opt.query_file = optarg; break;
      case 'E': opt.evaluate_file = optarg; break;
      case 'V': ensemble_arg = optarg; ensemble = true; break;
      case 'T': trajectory_steps = atoi(optarg); trajectory = true; break;
      case 'e': opt.sampled_arg = optarg; sampled = true; break;
      case 'N': opt.noisy_arg = optarg; noisy = true; break;
      case 'A': opt.actor_arg = optarg; actors = true; break;
      default: return 1;
    }
  }
  if (optind > argc - 1)
  {
    log(0, std::string("Usage: \n  ") + argv[0] + " [-v] [-s seed] [-r replicas] [-g gpus] [-t trials] [-l] [-q] [-p path=v1,v2,...]... [-n] [-k snapshot] [-K snapshot] [-Q observations] [-E states] [-V vote|mean] [-T steps] [-e epsilon|own|greedy] [-N sigma|own] [-A mean|binning[:bins]|data_center[:keep]|density[:r]] <yaml file> [yaml file...]");
    return 1;
  }
  if (opt.seed == 0)
  { // deployer.cpp:75-83: seed 0 means "from the clock"; the accelerated path wants reproducible runs
    log(0, "seed 0 (time-based seeding) is not supported; pass -s <seed>");
    return 1;
  }
  if (!sweep_args.empty())
  { // the grid: point-major, the Cartesian product of the axes in the order given (last fastest), every point -r times
    try
    {
      if (gpus > 1) throw Exception("-p: a parameter sweep runs on one GPU (-g " + std::to_string(gpus) + " is not built)");
      if (opt.replicas < 2) throw Exception("-p: -r (repetitions per point) must be >= 2: the standard deviation per point divides by repetitions - 1");
      std::vector<SweepAxis> axes;
      size_t points = 1;
      for (const std::string &a : sweep_args)
      {
        axes.push_back(parse_sweep_axis(a));
        for (size_t k = 0; k + 1 < axes.size(); ++k)
          if (axes[k].param == axes.back().param) throw Exception(std::string("-p: ") + kSweepPaths[axes.back().param] + " is given twice");
        points *= axes.back().values.size();
        if (points * (size_t)opt.replicas > (1u << 24)) throw Exception("-p: more than 2^24 clones");
      }
      const size_t R = (size_t)opt.replicas;
      for (size_t point = 0; point < points; ++point)
      {
        size_t rest = point;
        std::vector<size_t> at(axes.size());
        for (size_t a = axes.size(); a-- > 0;) { at[a] = rest % axes[a].values.size(); rest /= axes[a].values.size(); }
        for (size_t a = 0; a < axes.size(); ++a) opt.sweep[axes[a].param].insert(opt.sweep[axes[a].param].end(), R, axes[a].values[at[a]]);
      }
      opt.sweep_repetitions = opt.replicas;
      opt.replicas = (int)(points * R);
    }
    catch (Exception &e) { log(0, e.what()); return 1; }
  }
  if (!opt.snapshot_save.empty() || !opt.snapshot_load.empty())
  {
    try
    {
      if (!opt.snapshot_load.empty() && !sweep_args.empty()) throw Exception("-K together with -p: the per-replica values come from the snapshot");
      if (gpus > 1) throw Exception("-k / -K: a snapshot is one context on one GPU (-g " + std::to_string(gpus) + " is not built)");
    }
    catch (Exception &e) { log(0, e.what()); return 1; }
  }
  if (!opt.query_file.empty())
  { // the observation file is read, and -g refused, before any process is forked or any device looked for
    try
    {
      if (gpus > 1) throw Exception("-Q: a policy query runs on one GPU (-g " + std::to_string(gpus) + " is not built)");
      read_query_file(&opt);
    }
    catch (Exception &e) { log(0, e.what()); return 1; }
  }
  if (ensemble)
  { // -V needs -E's states and one of the two rules: refused before any process is forked or any device looked for
    if (ensemble_arg == "vote") opt.ensemble_rule = GRLX_ENSEMBLE_VOTE;
    else if (ensemble_arg == "mean") opt.ensemble_rule = GRLX_ENSEMBLE_MEAN_Q;
    else { log(0, "-V: unknown rule '" + ensemble_arg + "' (vote: the members' majority, mean: the argmax of their mean Q)"); return 1; }
    if (opt.evaluate_file.empty()) { log(0, "-V " + ensemble_arg + ": an ensemble evaluation needs the start states of -E <states file>"); return 1; }
  }
  if (trajectory)
  { // -T needs -E's states and a length the records can have; what -E refuses is refused here under -T's name
    if (trajectory_steps < 1 || trajectory_steps > GRLX_MAX_EPISODE_STEPS)
    { log(0, "-T " + std::to_string(trajectory_steps) + " is outside 1 ... GRLX_MAX_EPISODE_STEPS (" + std::to_string(GRLX_MAX_EPISODE_STEPS) + ")"); return 1; }
    if (opt.evaluate_file.empty()) { log(0, "-T " + std::to_string(trajectory_steps) + ": per-step trajectories need the start states of -E <states file>"); return 1; }
    if (gpus > 1) { log(0, "-T: trajectories of a policy evaluation run on one GPU (-g " + std::to_string(gpus) + " is not built)"); return 1; }
    if ((sweep_args.empty() ? opt.replicas : opt.sweep_repetitions) < 2)
    { log(0, "-T: -E needs -r >= 2: the standard deviation over the clones divides by n - 1"); return 1; }
    opt.trajectory_steps = trajectory_steps;
  }
  if (sampled)
  { // -e needs -E's states and a sampler; what -E refuses is refused here under -e's name, before any process is forked or any device looked for
    const std::string &arg = opt.sampled_arg;
    char *stop = nullptr;
    const double eps = strtod(arg.c_str(), &stop);
    if (arg == "greedy") { opt.sampled_sampler = GRLX_SAMPLER_GREEDY; opt.sampled_epsilon = 0; }
    else if (arg == "own") { opt.sampled_sampler = GRLX_SAMPLER_EPSILON_GREEDY; opt.sampled_epsilon = GRLX_EPSILON_OWN; }
    else if (!arg.empty() && *stop == 0 && eps >= 0. && eps <= 1.) { opt.sampled_sampler = GRLX_SAMPLER_EPSILON_GREEDY; opt.sampled_epsilon = eps; }
    else { log(0, "-e: '" + arg + "' is neither a number in [0, 1] nor 'own' (every clone's decayed epsilon) nor 'greedy' (the greedy sampler with its drawn tie break)"); return 1; }
    if (opt.evaluate_file.empty()) { log(0, "-e " + arg + ": a sampled evaluation needs the start states of -E <states file>"); return 1; }
    if (gpus > 1) { log(0, "-e: a sampled policy evaluation runs on one GPU (-g " + std::to_string(gpus) + " is not built)"); return 1; }
    if ((sweep_args.empty() ? opt.replicas : opt.sweep_repetitions) < 2)
    { log(0, "-e: -E needs -r >= 2: the standard deviation over the clones divides by n - 1"); return 1; }
  }
  if (noisy)
  { // -N needs -E's states and a standard deviation; what -E refuses is refused here under -N's name, before any process is forked or any device looked for
    const std::string &arg = opt.noisy_arg;
    char *stop = nullptr;
    const double sigma = strtod(arg.c_str(), &stop);
    if (arg == "own") opt.noisy_sigma = GRLX_SIGMA_OWN;
    else if (!arg.empty() && *stop == 0 && std::isfinite(sigma) && sigma >= 0.) opt.noisy_sigma = sigma;
    else { log(0, "-N: '" + arg + "' is neither a finite number >= 0 nor 'own' (every clone's decayed sigma)"); return 1; }
    opt.noisy = true;
    if (opt.evaluate_file.empty()) { log(0, "-N " + arg + ": a noisy evaluation needs the start states of -E <states file>"); return 1; }
    if (gpus > 1) { log(0, "-N: a noisy policy evaluation runs on one GPU (-g " + std::to_string(gpus) + " is not built)"); return 1; }
    if (!sweep_args.empty()) { log(0, "-N: a noisy evaluation is the actor-critic's, for which per-replica parameters (-p) are not built"); return 1; }
    if (opt.replicas < 2) { log(0, "-N: -E needs -r >= 2: the standard deviation over the clones divides by n - 1"); return 1; }
  }
  if (actors)
  { // -A needs -E's states, one of the four rules and a well-formed parameter: refused before any process is forked or any device looked for
    const std::string &arg = opt.actor_arg;
    const size_t colon = arg.find(':');
    const std::string name = arg.substr(0, colon), value = colon == std::string::npos ? "" : arg.substr(colon + 1);
    const bool given = colon != std::string::npos;
    char *stop = nullptr;
    if (name == "mean") opt.actor_rule = GRLX_ACTOR_ENSEMBLE_MEAN;
    else if (name == "binning") opt.actor_rule = GRLX_ACTOR_ENSEMBLE_BINNING;
    else if (name == "data_center") opt.actor_rule = GRLX_ACTOR_ENSEMBLE_DATA_CENTER;
    else if (name == "density") opt.actor_rule = GRLX_ACTOR_ENSEMBLE_DENSITY;
    else { log(0, "-A: unknown rule '" + name + "' (mean, binning[:bins], data_center[:keep], density[:r]: mapping/policy/multi's strategies)"); return 1; }
    if (given && opt.actor_rule == GRLX_ACTOR_ENSEMBLE_MEAN) { log(0, "-A " + arg + ": the rule mean takes no parameter"); return 1; }
    if (given && opt.actor_rule == GRLX_ACTOR_ENSEMBLE_DENSITY)
    {
      opt.actor_r = strtod(value.c_str(), &stop);
      if (value.empty() || *stop != 0 || !std::isfinite(opt.actor_r) || !(opt.actor_r > 0.))
      { log(0, "-A " + arg + ": '" + value + "' is not a finite radius above 0"); return 1; }
    }
    else if (given)
    {
      const long v = strtol(value.c_str(), &stop, 10);
      const long most = opt.actor_rule == GRLX_ACTOR_ENSEMBLE_BINNING ? 64 : 0x7fffffffl;
      if (value.empty() || *stop != 0 || v < 1 || v > most)
      { log(0, "-A " + arg + ": '" + value + "' is not " + (opt.actor_rule == GRLX_ACTOR_ENSEMBLE_BINNING ? "a number of bins in 1 ... 64" : "a number of members kept >= 1")); return 1; }
      opt.actor_bins = (int)v;
    }
    if (opt.evaluate_file.empty()) { log(0, "-A " + arg + ": an actor ensemble's evaluation needs the start states of -E <states file>"); return 1; }
    if (gpus > 1) { log(0, "-A: an actor ensemble's evaluation runs on one GPU (-g " + std::to_string(gpus) + " is not built)"); return 1; }
    if (!sweep_args.empty()) { log(0, "-A: an actor ensemble is the actor-critic's, for which per-replica parameters (-p) are not built"); return 1; }
  }
  if (!opt.evaluate_file.empty())
  { // likewise: the state file is read, and -g and -r 1 refused, before any process is forked or any device looked for
    try
    {
      if (gpus > 1) throw Exception("-E: a policy evaluation runs on one GPU (-g " + std::to_string(gpus) + " is not built)");
      if ((sweep_args.empty() ? opt.replicas : opt.sweep_repetitions) < 2)
        throw Exception("-E: -r must be >= 2: the standard deviation over the clones divides by n - 1");
      read_evaluate_file(&opt);
    }
    catch (Exception &e) { log(0, e.what()); return 1; }
  }
  if (opt.plan_only) gpus = 0;        // the plan is printed by this process, before anything touches HIP
  std::string id_file;
  if (gpus < 0 || gpus > 64) { log(0, "-g: between 1 and 64 processes"); return 1; }
  if (gpus >= 1)
  { // one process per GPU, forked BEFORE anything initialises HIP; each child narrows itself to its device
    std::ostringstream idn;
    idn << "/tmp/grlxd-" << getpid() << ".ncclid";
    id_file = idn.str();
    opt.world = gpus;
    if (gpus > 1)
    {
      std::vector<pid_t> kids;
      int rank = -1;
      for (int r = 0; r < gpus; ++r)
      {
        const pid_t pid = fork();
        if (pid < 0) { log(0, "fork failed"); return 1; }
        if (pid == 0) { rank = r; break; }
        kids.push_back(pid);
      }
      if (rank < 0)
      { // the parent: wait for the ranks in whatever order they end; the first failure ends the others (a rank that waits for a dead peer
        // inside the communicator's rendezvous would wait for ever)
        int bad = 0;
        for (size_t left = kids.size(); left > 0; --left)
        {
          int st = 0;
          const pid_t done = waitpid(-1, &st, 0);
          if (done < 0) { bad++; break; }
          if (!WIFEXITED(st) || WEXITSTATUS(st) != 0)
          {
            if (bad++ == 0)
              for (pid_t k : kids)
                if (k != done) kill(k, SIGTERM);
          }
        }
        unlink(id_file.c_str());
        if (bad) log(0, std::to_string(bad) + " of " + std::to_string(gpus) + " ranks failed");
        return bad ? 1 : 0;
      }
      opt.rank = rank;
    }
    try { setenv("HIP_VISIBLE_DEVICES", device_for_rank(opt.rank).c_str(), 1); }
    catch (Exception &e) { log(0, e.what()); return 1; }
  }
  std::unique_ptr<CurveReducer> reducer;
  try
  {
    if (gpus >= 1)
    {
      reducer.reset(make_rccl_reducer(opt.rank, opt.world, id_file));
      opt.reducer = reducer.get();
      log(2, "rank " + std::to_string(opt.rank) + " of " + std::to_string(opt.world) + ": communicator ready");
    }
    YamlNode root;
    for (; optind < argc; ++optind)
    {
      log(2, std::string("Loading configuration from '") + argv[optind] + "'");
      std::ifstream ifs(argv[optind]);
      if (!ifs) { log(0, std::string("Could not load configuration '") + argv[optind] + "'"); return 1; }
      std::stringstream ss;
      ss << ifs.rdbuf();
      merge_yaml(root, parse_yaml(ss.str()));
    }
    if (trials_override >= 0)
      for (auto &kv : root.children)
        if (kv.first == "experiment")
          for (auto &p : kv.second.children)
          {
            if (p.first == "trials") p.second.scalar = std::to_string(trials_override);
            if (p.first == "experiment")                       // experiment/multi { experiment: experiment/online_learning }
              for (auto &q : p.second.children)
                if (q.first == "trials") q.second.scalar = std::to_string(trials_override);
          }
    log(2, "Instantiating configuration");
    std::unique_ptr<Configurator> tree = instantiate(root);
    Configurator *expconf = tree->child("experiment");
    if (!expconf || !expconf->is_object) { log(0, "YAML configuration does not specify an experiment"); return 1; }
    Experiment *experiment = dynamic_cast<Experiment *>(expconf->object.get());
    if (!experiment) { log(0, "Specified experiment has wrong type"); return 1; }
    log(2, "Starting experiment");
    experiment->run(opt);
    log(2, "Cleaning up");
  }
  catch (Exception &e)
  {
    log(0, e.what());
    return 1;
  }
  return 0;
}
