// objects.h -- what the deployer needs to know about the experiment object.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "configurable.h"

namespace grlx_host {

struct CurveReducer;            // multi_gpu.h
struct RunOptions {
  int64_t seed = 1;             // deployer -s (replica i uses seed + i)
  int replicas = 1;             // clones of the experiment (experiment/multi analogue)
  // `grlxd -g N`: this process is rank `rank` of `world`, one per GPU.  Its replicas are the clones rank * replicas .. + replicas - 1 of the
  // whole job (seeds and "@i" identities count over all ranks); after every run the ranks reduce their learning curves with ONE all-reduce
  // (reducer->all_reduce_sum over grlx_curve_stats' device buffer) and rank 0 writes <output>-<run>-mean.txt.
  int rank = 0, world = 1;
  CurveReducer *reducer = nullptr;
  int table_log2_capacity = 0;
  bool legacy_rows = false;     // 3-column rows as in the reference's committed golden files
  bool print_rows = true;
  // `grlxd -p <path>=v1,v2,...`: a grid sweep over predictor alpha / gamma / lambda and the sampler's epsilon -- the study of the reference's
  // bin/grlo (bin/optimize.yaml) as the replicas of ONE device context.  sweep[k] (k = GRLX_PARAM_*) is empty (the yaml's value for every
  // clone) or holds the value of every clone; clone i = point * sweep_repetitions + k, the points being the Cartesian product of the
  // axes in the order given, the last one fastest.  replicas = points * sweep_repetitions.  After every run rank 0 writes
  // <output>-<run>-sweep.txt: per point its index, the four values, and n / avg / stddev / stderr of the clones' simple regret as
  // bin/grlo prints them.
  std::vector<double> sweep[4];
  int sweep_repetitions = 0;    // > 0: a sweep
  bool plan_only = false;       // `grlxd -n`: print one line per clone (i seed alpha gamma lambda epsilon) and run nothing
  // exact resume (grlx_snapshot_save / _load): `grlxd -k FILE` writes the context's snapshot when the trial loop of the run ends (and reserves
  // at least kSnapshotRows test rows, so that a continuation has room for its own); `grlxd -K FILE` starts from one: the trial loop continues at
  // the snapshot's trial count up to `trials:` / -t, and the output files are written whole -- the rows are in the snapshot
  std::string snapshot_save, snapshot_load;
  // `grlxd -Q FILE`: after the last trial of every run of an experiment/online_learning with a Q agent, the policy is queried at the
  // observations of FILE (one per line, whitespace-separated numbers, `#` comments; read by read_query_file before any device is looked
  // for) with grlx_query_ensemble and rank 0 writes <output>-<run>-policy.txt: per observation its coordinates, mean and standard deviation
  // (n - 1) of QPolicy::value over the clones, the votes per action and the majority action's value (the lowest index wins a tie), in the
  // stream format of the rows files.  With -p: one line per (point, observation), the point's index first, the groups being the repetitions.
  std::string query_file;
  std::vector<double> query_obs;    // [query_rows][query_cols]
  int query_rows = 0, query_cols = 0;
  // `grlxd -E FILE`: after the last trial of every run of an experiment/online_learning, one greedy episode per (clone, start state) with
  // grlx_evaluate from the MODEL states of FILE (one per line, as many columns as grlx_env_dims reports state dimensions -- the time
  // included --, `#` comments; read by read_evaluate_file before any device is looked for), and rank 0 writes <output>-<run>-returns.txt:
  // per start state one line "mean sd mean_steps n0 n1 n2 n3 ties" (%.17g) -- mean and standard deviation (n - 1, two passes) of the return
  // and the mean number of steps over the clones, the number of clones whose episode ended with terminal code 0 (cut at
  // GRLX_MAX_EPISODE_STEPS), 1 (timed out), 2 (absorbing), 3 (left the math domain), and the summed ties; every sum on the host in
  // ascending clone order.  With -p: one line per (point, start state), the point's index first, over the repetitions of the point.
  std::string evaluate_file;
  std::vector<double> evaluate_states;    // [evaluate_rows][evaluate_cols]
  int evaluate_rows = 0, evaluate_cols = 0;
  // `grlxd -E FILE -V vote|mean`: besides the unchanged returns file, one episode per (group, start state) with grlx_evaluate_ensemble, the
  // group being all clones, with -p the repetitions of a point; rank 0 writes <output>-<run>-ensemble.txt: per start state one line
  // "ret disc steps terminal ties member_ties agreement" (%.17g), agreement = grlx_evaluate_ensemble's divided by steps * group.  With -p:
  // one line per (point, start state), the point's index first.  -1 = no -V; else GRLX_ENSEMBLE_VOTE / GRLX_ENSEMBLE_MEAN_Q.
  int ensemble_rule = -1;
  // `grlxd -E FILE -T STEPS`: besides the unchanged returns file, the steps of those episodes up to STEPS each (grlx_evaluate_trajectory,
  // 1 ... GRLX_MAX_EPISODE_STEPS); rank 0 writes <output>-<run>-trajectories.txt: one line per (clone, start state, step taken), ascending,
  // "clone start step" and the words of the record (include/grlx.h: GRLX_TRAJ_*) -- action index, number of maxima and terminal code as
  // integers, the others %.17g.  With -V also <output>-<run>-ensemble-trajectories.txt (grlx_evaluate_ensemble_trajectory), its lines
  // beginning "group start step".  The episodes of the returns and ensemble files are not cut at STEPS.  0 = no -T.
  int trajectory_steps = 0;
  // `grlxd -E FILE -e <epsilon | own | greedy>`: besides the unchanged returns file, one SAMPLED episode per (clone, start state) with
  // grlx_evaluate_sampled -- the epsilon-greedy sampler on a number in [0, 1] or on every clone's own decayed epsilon, or the greedy sampler
  // with its drawn tie break -- on the streams of grlx_episode_streams(-s seed, pair 0 ...); rank 0 writes <output>-<run>-sampled.txt: per
  // start state one line "mean sd mean_steps n0 n1 n2 n3 ties explored", the returns file's columns and the summed explored steps.  With -p:
  // one line per (point, start state), the point's index first.  With -T also <output>-<run>-sampled-trajectories.txt
  // (grlx_evaluate_sampled_trajectory), the trajectories file's lines with one word more, the record's last: 1 where the step explored.
  // sampled_sampler: -1 = no -e; else GRLX_SAMPLER_*.  sampled_epsilon: the number, or GRLX_EPSILON_OWN.
  int sampled_sampler = -1;
  double sampled_epsilon = 0;
  std::string sampled_arg;
  // `grlxd -E FILE -N <sigma | own>`: besides the unchanged returns file, one NOISY episode per (clone, start state) of an actor-critic with
  // grlx_evaluate_noisy -- the exploring policy on a standard deviation >= 0 or on every clone's own decayed sigma, on the configuration's
  // theta -- on the streams of grlx_episode_stream_words(-s seed, pair 0 ...), from a noise state of 0; rank 0 writes
  // <output>-<run>-noisy.txt: per start state one line "mean sd mean_steps n0 n1 n2 n3 ties clipped", the returns file's columns (ties is
  // 0: a continuous action has none) and the summed clipped steps.  With -T also <output>-<run>-noisy-trajectories.txt
  // (grlx_evaluate_noisy_trajectory), the trajectories file's lines with two words more, the record's last: the noise state after the
  // step, 1 where the step clipped.  noisy_sigma: the number, or GRLX_SIGMA_OWN.
  bool noisy = false;
  double noisy_sigma = 0;
  std::string noisy_arg;
  // -A mean|binning[:bins]|data_center[:keep]|density[:r] (needs -E, an actor-critic): also one episode per start state of the ensemble of ALL
  // clones on the members' combined action (grlx_evaluate_actor_ensemble).  <output>-<run>-actor-ensemble.txt: per start state one line
  // "ret disc steps terminal ties kept spread".  With -T also <output>-<run>-actor-ensemble-trajectories.txt
  // (grlx_evaluate_actor_ensemble_trajectory): the trajectories file's lines for group 0, with the record's two last words, the step's kept
  // and spread.  actor_rule: GRLX_ACTOR_ENSEMBLE_*, -1 without -A.
  int actor_rule = -1;
  int actor_bins = 10;
  double actor_r = 0.001;
  std::string actor_arg;
};
// ... the same for opt.evaluate_file -> opt.evaluate_states / _rows / _cols (messages begin with -E)
void read_evaluate_file(RunOptions *opt);
// fills opt.query_obs / _rows / _cols from opt.query_file; Exception for a missing or empty file, a token that is no finite number, rows of
// different lengths
void read_query_file(RunOptions *opt);

// Environment::step (environment.h:48-51 -> ModeledEnvironment::step, modeled.cpp:160-213) for a batch of instances:
// state[n][S] is advanced in place; obs[n][D], reward[n], terminal[n].  Forwards to grlx_env_step (HIP kernel).
struct Environment : Configurable {
  virtual void dims(int *state_dims, int *obs_dims) const = 0;
  virtual void step(double *state, const double *action, int n, double *obs, double *reward, int32_t *terminal) const = 0;
};

// Projector::project (projector.h:55-69 -> TileCodingProjector::_project, tile_coding.cpp:103-149) for a batch of
// inputs in[n][dims] -> out[n][tilings] reference slot indices.  Forwards to grlx_project (HIP kernel).
struct Projector : Configurable {
  virtual int n_tilings() const = 0;
  virtual int n_dims() const = 0;
  virtual void project(const double *in, int n, uint32_t *out) const = 0;
};

// Representation::read / write / update (representation.h:60-83 -> LinearRepresentation, linear.cpp:136-216) for rows of
// projections idx[n][16] (reference slot indices, as Projector::project returns them), applied in row order.  The parameter
// vector lives on the GPU: the object owns a one-replica context whose table it is -- drawn from srand48(seed) the way
// LinearRepresentation::configure draws it as the first user of a fresh process -- and forwards to grlx_read / grlx_write /
// grlx_update (HIP kernel table_op_kernel).  target[n] / delta[n]: one output per row (outputs = 1).
struct Representation : Configurable {
  virtual void reset(int64_t seed) = 0;
  virtual void read(const uint32_t *idx, int n, double *out) = 0;
  virtual void write(const uint32_t *idx, int n, const double *target, double alpha) = 0;
  virtual void update(const uint32_t *idx, int n, const double *delta) = 0;
};

// Experiment::run (experiment.h:44) -> learning curve of replica 0
struct Experiment : Configurable {
  virtual std::vector<double> run(const RunOptions &opt) = 0;
};
struct OnlineLearningExperiment : Experiment {};

// The per-step side of the plug-in API: the experiment's environment and agents as objects a caller steps itself -- the loop of
// OnlineLearningExperiment::run (online_learning.cpp:172-213) stays with the caller, one side (or both) runs on the GPU, every call
// serves all replicas of the experiment's device context (rows of [replicas]; `active`: NULL or a mask of the replicas taking part).
//   Environment::start / step  (environment.h:48-51)  -> grlx_env_start / grlx_env_advance
//   Agent::start / step / end  (agent.h:44-56)        -> grlx_agent_start / _step / _end; agent/td is the learning agent, agent/fixed the test agent
struct StepwiseEnvironment {
  virtual ~StepwiseEnvironment() {}
  virtual void start(int test, const int32_t *active, double *obs) = 0;
  virtual void step(const int32_t *active, const double *action, double *obs, double *reward, int32_t *terminal) = 0;
};
struct StepwiseAgent {
  virtual ~StepwiseAgent() {}
  virtual void start(const int32_t *active, const double *obs, double *action) = 0;
  virtual void step(const int32_t *active, double tau, const double *obs, const double *reward, const int32_t *terminal, double *action) = 0;
  virtual void end(const int32_t *active, double tau, const double *obs, const double *reward) = 0;
};
// experiment/online_learning as the owner of the device context its objects step on
struct StepwiseExperiment {
  virtual ~StepwiseExperiment() {}
  virtual void open(const RunOptions &opt) = 0;                 // instantiate on the GPU (grlx_create of the lowered graph)
  virtual void close() = 0;
  virtual int replicas() const = 0;
  virtual int obs_dims() const = 0;
  virtual int test_interval_of() const = 0;
  virtual StepwiseEnvironment *stepwise_environment() = 0;
  virtual StepwiseAgent *stepwise_agent() = 0;
  virtual StepwiseAgent *stepwise_test_agent() = 0;
};

} // namespace grlx_host
