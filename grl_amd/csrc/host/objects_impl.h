// objects_impl.h -- private to the object units (objects_*.cpp): the reference's plug-in classes on the hot path, as configuration
// descriptors with the same TYPEINFO strings, parameter names, defaults and bad_param conditions, and the owners of what the C ABI
// (include/grlx.h) hands out.  Only what crosses a unit is declared here; the deployer and grlx_ops see objects.h alone.
// Nothing here computes the algorithm on the CPU: a graph the fused kernels do not implement is refused.
#pragma once
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/grlx.h"
#include "configurable.h"
#include "objects.h"
#include "report_rules.h"

namespace grlx_host {

using VecD = std::vector<double>;
static const double kPi = 3.14159265358979323846;

// ---------------------------------------------------------------- owners ---
// A context lives exactly as long as its owner: the two deleters are the only callers of grlx_destroy / grlx_fqi_destroy.
struct CtxDeleter { void operator()(grlx_ctx *ctx) const { grlx_destroy(ctx); } };
using CtxOwner = std::unique_ptr<grlx_ctx, CtxDeleter>;
struct FqiCtxDeleter { void operator()(grlx_fqi_ctx *ctx) const { grlx_fqi_destroy(ctx); } };
using FqiCtxOwner = std::unique_ptr<grlx_fqi_ctx, FqiCtxDeleter>;

// a status of the C ABI that is not GRLX_OK becomes an Exception with the ABI's message.  The exception is built here, before
// unwinding releases any owner, so the message is read before a context is destroyed.
inline void check(int status, const std::string &prefix = "")
{
  if (status != GRLX_OK) throw Exception(prefix + grlx_last_error());
}
inline CtxOwner create_context(const grlx_config &c, const int64_t *seeds, const std::string &prefix = "")
{
  grlx_ctx *ctx = nullptr;
  check(grlx_create(&c, seeds, &ctx), prefix);
  return CtxOwner(ctx);
}

// ------------------------------------------------------------ environment ---  (objects_env.cpp)
struct Dynamics : Configurable { virtual int env_id() const = 0; };
struct Task : Configurable {
  virtual int env_id() const = 0;
  double timeout = 0, randomization = 0;
};
struct Model : Configurable {
  double control_step = 0.05;
  int integration_steps = 5;
  virtual int env_id() const = 0;
};

// model/dynamical (modeled.cpp:234-252)
struct DynamicalModel : Model {
  GRLX_TYPEINFO("model/dynamical")
  Dynamics *dynamics = nullptr;
  int env_id() const override { return dynamics ? dynamics->env_id() : -1; }
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

// environment/modeled (modeled.cpp:35-119)
struct ModeledEnvironment : Environment {
  GRLX_TYPEINFO("environment/modeled")
  Model *model = nullptr;
  Task *task = nullptr;
  int discrete_time = 1;
  Configurable *exporter = nullptr;     // optional exporter/csv for the transition log with the model state (modeled.cpp:67-71)
  void lower_env(grlx_config *c) const;                 // model + task -> the environment fields of a grlx_config
  void dims(int *state_dims, int *obs_dims) const override;
  void step(double *state, const double *action, int n, double *obs, double *reward, int32_t *terminal) const override;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

// ------------------------------------------------------------------ agent ---  (objects_agent.cpp)
// discretizer/uniform (uniform.cpp:34-95)
struct UniformDiscretizer : Configurable {
  GRLX_TYPEINFO("discretizer/uniform")
  VecD min, max, steps;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

// projector/tile_coding (tile_coding.cpp:34-80)
struct TileCodingProjector : Projector {
  GRLX_TYPEINFO("projector/tile_coding")
  int tilings = 16, memory = 8 * 1024 * 1024, safe = 0;
  VecD resolution, wrapping;
  int n_tilings() const override { return tilings; }
  int n_dims() const override { return (int)resolution.size(); }
  void lower(grlx_tile_spec *t) const;                  // the projector as the C ABI takes it
  void project(const double *in, int n, uint32_t *out) const override;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

// representation/parameterized/linear (linear.cpp:34-101)
struct LinearRepresentation : Representation {
  GRLX_TYPEINFO("representation/parameterized/linear")
  VecD init_min, init_max, output_min, output_max;
  int memory = 8 * 1024 * 1024, outputs = 1, limit = 1, interval = 0;
  double tau = 1;
  // the stand-alone use of the object (Representation interface): a private one-replica context holds the parameters
  CtxOwner own;
  grlx_ctx *context();
  void reset(int64_t seed) override;
  void read(const uint32_t *idx, int n, double *out) override;
  void write(const uint32_t *idx, int n, const double *target, double alpha) override;
  void update(const uint32_t *idx, int n, const double *delta) override;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

// sampler/greedy, sampler/epsilon_greedy (greedy.cpp:34-130)
struct GreedySampler : Configurable {
  GRLX_TYPEINFO("sampler/greedy")
  virtual bool explores() const { return false; }
};
struct EpsilonGreedySampler : GreedySampler {
  GRLX_TYPEINFO("sampler/epsilon_greedy")
  VecD epsilon; double decay_rate = 1, decay_min = 0;
  bool explores() const override { return true; }
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

struct Policy : Configurable {};

// mapping/policy/action (action.cpp:38-91)
struct ActionPolicy : Policy {
  GRLX_TYPEINFO("mapping/policy/action")
  VecD sigma, theta, min, max; double decay_rate = 1, decay_min = 0;
  TileCodingProjector *projector = nullptr; LinearRepresentation *representation = nullptr;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

// mapping/policy/discrete/value/q (q.cpp:35-52); the reference's own test yaml still says policy/discrete/q
struct QPolicy : Policy {
  GRLX_TYPEINFO("mapping/policy/discrete/value/q")
  UniformDiscretizer *discretizer = nullptr; TileCodingProjector *projector = nullptr;
  LinearRepresentation *representation = nullptr; GreedySampler *sampler = nullptr;
  Configurable *any_projector = nullptr, *any_representation = nullptr;     // whatever the yaml gave (the batch path: normalizing projector, iterative ANN)
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

struct Trace : Configurable { virtual int kind() const = 0; };
struct Predictor : Configurable {};

// predictor/critic/sarsa (sarsa.cpp:35-60), predictor/critic/q (advantage.cpp:35-62), .../advantage, .../expected_sarsa, .../qv
struct TDPredictorBase : Predictor {
  double alpha = 0.2, gamma = 0.97, lambda = 0.65, kappa = 0;
  TileCodingProjector *projector = nullptr; LinearRepresentation *representation = nullptr; Trace *trace = nullptr;
  virtual int agent_id() const = 0;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};
// predictor/critic/expected_sarsa (sarsa.cpp:134-165): the target policy must be the learning policy
struct ExpectedSARSAPredictor : TDPredictorBase {
  GRLX_TYPEINFO("predictor/critic/expected_sarsa")
  Configurable *target_policy = nullptr;
  int agent_id() const override { return GRLX_AGENT_EXPECTED_SARSA; }
  void request(const std::string &role, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};
// predictor/critic/qv (qv.cpp:35-64): Q(s,a) and V(s) tables, the trace on V
struct QVPredictor : TDPredictorBase {
  GRLX_TYPEINFO("predictor/critic/qv")
  double beta = 0.1;
  TileCodingProjector *v_projector = nullptr; LinearRepresentation *v_representation = nullptr;
  int agent_id() const override { return GRLX_AGENT_QV; }
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};
// predictor/critic/td (predictors/td.cpp:35-58): V(s) critic with a trace
struct VPredictor : Predictor {
  GRLX_TYPEINFO("predictor/critic/td")
  double alpha = 0.2, gamma = 0.97, lambda = 0.65;
  TileCodingProjector *projector = nullptr; LinearRepresentation *representation = nullptr; Trace *trace = nullptr;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};
// predictor/ac/action (ac.cpp:36-70)
struct ActionACPredictor : Predictor {
  GRLX_TYPEINFO("predictor/ac/action")
  double alpha = 0.01; std::string update_method = "proportional"; VecD step_limit;
  TileCodingProjector *projector = nullptr; LinearRepresentation *representation = nullptr; VPredictor *critic = nullptr;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

// agent/td (td.cpp:34-48), agent/fixed (fixed.cpp:34-45)
struct TDAgent : Configurable {
  GRLX_TYPEINFO("agent/td")
  Policy *policy = nullptr; Predictor *predictor = nullptr;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};
struct FixedAgent : Configurable {
  GRLX_TYPEINFO("agent/fixed")
  Policy *policy = nullptr;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
};

// --------------------------------------------------------------- exporter ---  (objects_csv.cpp)
// exporter/csv (exporters/csv.cpp:37-206, exporter.h:62-95): comma-separated transition log.
// Same parameters, file naming (<file>-<variant>-<run counter>.csv), header styles and number
// format; fed from the device's per-step taps after a run instead of once per step.
struct CSVExporter : Configurable {
  GRLX_TYPEINFO("exporter/csv")
  std::string file, fields, style = "line", variant = "all";
  int enabled = 1, offset = 0;
  std::vector<std::string> headers;
  std::vector<size_t> order;
  std::ofstream stream;
  bool header_due = true;
  std::map<std::string, int> counter;
  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
  void init(const std::vector<std::string> &h);         // register the columns the caller will supply and resolve `fields` against them
  void open(const std::string &which, bool append);     // a non-appending open starts the next numbered file of the variant
  void write(const std::vector<std::vector<double>> &vars);
  void close() { if (stream.is_open()) stream.close(); }
};
// the two transition logs of a run, from the taps of replica 0 in device order
void write_environment_log(CSVExporter *out, const std::vector<grlx_tap> &taps, int state_dims, int obs_dims, double control_step);
void write_experiment_log(CSVExporter *out, const std::vector<grlx_tap> &taps, int obs_dims);

// ------------------------------------------------------------- experiment ---  (objects_online.cpp, objects_reports.cpp)
// The experiment's objects stepped by the caller: thin forwards to the per-step entry points of the C ABI on the experiment's context
struct ContextEnvironment : StepwiseEnvironment {
  grlx_ctx *ctx = nullptr;
  void start(int test, const int32_t *active, double *obs) override;
  void step(const int32_t *active, const double *action, double *obs, double *reward, int32_t *terminal) override;
};
struct ContextAgent : StepwiseAgent {
  grlx_ctx *ctx = nullptr;
  int test = 0;                                     // 0: agent/td, 1: agent/fixed (the test agent)
  void start(const int32_t *active, const double *obs, double *action) override;
  void step(const int32_t *active, double tau, const double *obs, const double *reward, const int32_t *terminal, double *action) override;
  void end(const int32_t *active, double tau, const double *obs, const double *reward) override;
};

// everything OnlineLearningExperimentImpl::run decides, or refuses, before a device is asked for
struct RunPlan {
  const RunOptions *opt = nullptr;
  grlx_config c;
  bool by_trial = false;            // one launch per trial: a steps budget, save_every: test | trial
  bool snap_save = false, snap_load = false, sweep = false, query = false, evaluate = false;
  bool many = false;                // more than one clone in the whole job: output names carry "@i"
  int trial_cap = 0;                // trials a run can take
  int first_trial = 0;              // -K: the trial loop continues where the snapshot's stopped
  int first_clone = 0;              // `grlxd -g N`: this rank's clones among those of the whole job
  int group = 0;                    // clones behind one figure of -Q / -E / -V: the repetitions of a sweep's point, else all of them
  int state_dims = 0, obs_dims = 0;
  std::vector<char> snapshot;       // -K: the file's bytes, released once they are loaded
};
// rows of one run as the reports share them
struct RunRows {
  int n = 0;                        // rows every clone wrote
  double wall = 0;                  // seconds of the trial loop (and the snapshot)
  std::vector<double> regret;       // a sweep: the simple regret of every clone
};

struct OnlineLearningExperimentImpl : OnlineLearningExperiment, StepwiseExperiment {
  GRLX_TYPEINFO("experiment/online_learning")
  // ---- StepwiseExperiment: the graph instantiated on the GPU, its environment and agents stepped by the caller
  CtxOwner step_ctx;
  grlx_config step_cfg;
  ContextEnvironment step_env;
  ContextAgent step_agent, step_test_agent;
  void open(const RunOptions &opt) override;
  void close() override { step_ctx = nullptr; }
  int replicas() const override { return step_cfg.n_replicas; }
  int obs_dims() const override { int s = 0, d = 0; grlx_env_dims(step_cfg.env, &s, &d); return d; }
  int test_interval_of() const override { return test_interval; }
  StepwiseEnvironment *stepwise_environment() override { return &step_env; }
  StepwiseAgent *stepwise_agent() override { return &step_agent; }
  StepwiseAgent *stepwise_test_agent() override { return &step_test_agent; }

  int runs = 1, run_offset = 0, trials = 0, steps = 0, test_interval = -1, test_trials = 1;
  std::string output, load_file, save_every;
  ModeledEnvironment *environment = nullptr; TDAgent *agent = nullptr; FixedAgent *test_agent = nullptr;
  CSVExporter *exporter = nullptr, *env_exporter = nullptr;

  void request(const std::string &, ConfigurationRequest *config) override;
  void configure(Configuration &config) override;
  // lower the instantiated graph to the C ABI's grlx_config; every assumption the fused kernels make is checked
  void lower(grlx_config *c) const;
  int order_of(const Configurable *o) const;
  // the parameterized representations of the agent in table order: 0 = Q / critic, 1 = actor / V
  std::vector<const Configurable *> representations() const;
  std::vector<double> run(const RunOptions &opt) override;

  // ---- the stages of run(), in the order it performs them; none owns anything
  RunPlan plan(const RunOptions &opt) const;
  void print_plan(const RunPlan &p) const;
  void apply_sweep(const RunPlan &p, grlx_ctx *ctx) const;
  void load_snapshot(RunPlan &p, grlx_ctx *ctx) const;
  void load_policy(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void trial_loop(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void save_snapshot(const RunPlan &p, grlx_ctx *ctx) const;
  std::vector<grlx_tap> read_taps(const RunPlan &p, grlx_ctx *ctx) const;
  void save_policy(const RunPlan &p, grlx_ctx *ctx, const std::string &base) const;
  // ---- the reports of a run (objects_reports.cpp)
  void write_rows(const RunPlan &p, grlx_ctx *ctx, int run, RunRows *rows, std::vector<double> *curve) const;
  void write_sweep_file(const RunPlan &p, int run, const RunRows &rows) const;
  void write_policy_file(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void write_returns_file(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void write_ensemble_file(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void write_trajectory_files(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void write_sampled_files(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void write_noisy_files(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void write_actor_ensemble_files(const RunPlan &p, grlx_ctx *ctx, int run) const;
  void write_mean_file(const RunPlan &p, grlx_ctx *ctx, int run, const RunRows &rows) const;
};

} // namespace grlx_host
