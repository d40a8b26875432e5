// objects_online.cpp -- experiment/online_learning: its parameters, the lowering of the instantiated graph to a grlx_config, the
// objects a caller steps itself, and run() as the sequence of stages it performs.  The report files are objects_reports.cpp's.
#include <chrono>
#include <cmath>
#include <fstream>
#include <iostream>
#include <sstream>

#include "objects_impl.h"

namespace grlx_host {

using OnlineImpl = OnlineLearningExperimentImpl;

void OnlineImpl::request(const std::string &, ConfigurationRequest *config)
{ // online_learning.cpp:40-62
  config->push_back(CRP("runs", "Number of separate learning runs to perform", 1));
  config->push_back(CRP("run_offset", "Run offset to start at", 0));
  config->push_back(CRP("trials", "Number of episodes per learning run", 0));
  config->push_back(CRP("steps", "Number of steps per learning run", 0));
  config->push_back(CRP("rate", "Control step frequency in Hz", 0, CRP::Online));
  config->push_back(CRP("test_interval", "Number of episodes in between test trials", -1));
  config->push_back(CRP("test_trials", "Number of test trials per interval", 1));
  config->push_back(CRP("output", "Output base filename", std::string()));
  config->push_back(CRP("environment", "environment", "Environment in which the agent acts", (Configurable *)nullptr));
  config->push_back(CRP("agent", "agent", "Agent", (Configurable *)nullptr));
  config->push_back(CRP("test_agent", "agent", "Agent to use in test trials", (Configurable *)nullptr, true));
  config->push_back(CRP("exporter", "exporter", "Optional exporter for transition log", (Configurable *)nullptr, true));
  config->push_back(CRP("load_file", "Load policy filename", std::string()));
  config->push_back(CRP("save_every", "Save policy to 'output' at the end of event", std::string("never")));
}
void OnlineImpl::configure(Configuration &config)
{
  runs = config["runs"]; run_offset = config["run_offset"]; trials = config["trials"]; steps = config["steps"];
  test_interval = config["test_interval"]; test_trials = config["test_trials"];
  output = config["output"].str(); load_file = config["load_file"].str(); save_every = config["save_every"].str();
  environment = dynamic_cast<ModeledEnvironment *>(config["environment"].ptr());
  agent = dynamic_cast<TDAgent *>(config["agent"].ptr());
  test_agent = dynamic_cast<FixedAgent *>(config["test_agent"].ptr());
  if (runs < 1) throw bad_param("experiment/online_learning:runs");
  if (test_interval < -1) throw bad_param("experiment/online_learning:test_interval");
  if (test_interval >= 0 && !config["test_agent"].ptr()) throw bad_param("experiment/online_learning:test_agent");   // :100-101
  if (!environment || !agent || (config["test_agent"].ptr() && !test_agent))
    throw Exception(path() + ": the accelerated path needs environment/modeled, agent/td and agent/fixed");
  if (save_every != "never" && save_every != "run" && save_every != "test" && save_every != "trial")
    throw bad_param("experiment/online_learning:save_every");
  if (steps < 0) throw bad_param("experiment/online_learning:steps");
  if (test_trials < 1) throw bad_param("experiment/online_learning:test_trials");
  if ((int)config["rate"] != 0)
    throw Exception(path() + ": rate (wall-clock pacing) is outside the accelerated path");
  exporter = dynamic_cast<CSVExporter *>(config["exporter"].ptr());
  if (config["exporter"].ptr() && !exporter) throw Exception(path() + ": only exporter/csv is available on the accelerated path");
  if (exporter) exporter->init({"time", "observation", "action", "reward", "terminal"});      // online_learning.cpp:74-75
  env_exporter = dynamic_cast<CSVExporter *>(environment->exporter);
  if (environment->exporter && !env_exporter) throw Exception(environment->path() + ": only exporter/csv is available on the accelerated path");
  if (env_exporter) env_exporter->init({"time", "state", "observation", "action", "reward", "terminal"});   // modeled.cpp:70-71
}

// lower the instantiated graph to the C ABI's grlx_config; every assumption the fused kernels make is checked
static void lower_linear(const LinearRepresentation *r, const TileCodingProjector *p, grlx_linear_spec *l)
{
  if (r->outputs != 1) throw Exception(r->path() + ": outputs must be 1");
  if (r->memory != p->memory) throw bad_param("representation/parameterized/linear:memory (or matching projector)");
  l->init_min = r->init_min[0]; l->init_max = r->init_max[0];
  l->output_min = r->output_min[0]; l->output_max = r->output_max[0];
  l->limit = r->limit;
}
int OnlineImpl::order_of(const Configurable *o) const
{
  int k = 0;
  for (Configurator *n : instantiate_order()) { if (n->object.get() == o) return k; ++k; }
  return -1;
}

void OnlineImpl::lower(grlx_config *c) const
{
  grlx_config_pendulum_sarsa(c);
  c->test_interval = test_interval;
  c->test_trials = test_trials;
  environment->lower_env(c);

  if (const ActionACPredictor *ac = dynamic_cast<const ActionACPredictor *>(agent->predictor))
  { // ---- actor-critic (cfg/cart_pole/ac_tc.yaml)
    const ActionPolicy *pol = dynamic_cast<const ActionPolicy *>(agent->policy);
    const ActionPolicy *tpol = test_agent ? dynamic_cast<const ActionPolicy *>(test_agent->policy) : nullptr;
    if (!pol || (test_agent && !tpol)) throw Exception(path() + ": predictor/ac/action needs mapping/policy/action policies");
    if (ac->projector != pol->projector || ac->representation != pol->representation)
      throw Exception(ac->path() + ": actor predictor and policy must share projector and representation");
    if (tpol && (tpol->projector != pol->projector || tpol->representation != pol->representation))
      throw Exception(test_agent->path() + ": the test policy must share projector and representation with the learning policy");
    if (tpol && tpol->sigma[0] != 0) throw Exception(tpol->path() + ": the test policy must be noise-free (sigma: [])");
    const VPredictor *cr = ac->critic;
    if (cr->representation == pol->representation) throw Exception(cr->path() + ": actor and critic need separate tables");
    // both tables draw their initial weights from one thread-local stream: actor first
    if (!(order_of(pol->representation) >= 0 && order_of(pol->representation) < order_of(cr->representation)))
      throw Exception(path() + ": this yaml instantiates the actor/critic tables in an order the fused kernel does not reproduce");
    c->agent = GRLX_AGENT_AC;
    c->action_min = pol->min[0]; c->action_max = pol->max[0]; c->action_steps = 0;
    cr->projector->lower(&c->projector);
    lower_linear(cr->representation, cr->projector, &c->representation);
    pol->projector->lower(&c->actor_projector);
    lower_linear(pol->representation, pol->projector, &c->actor_representation);
    if (cr->representation->interval || pol->representation->interval)
      throw Exception(path() + ": target networks (interval) are built for predictor/critic/sarsa and predictor/critic/q only");
    c->alpha = cr->alpha; c->gamma = cr->gamma; c->lambda = cr->lambda;
    c->trace = cr->trace ? cr->trace->kind() : GRLX_TRACE_NONE;
    c->actor_alpha = ac->alpha;
    c->sigma = pol->sigma[0]; c->theta = pol->theta[0];
    c->ac_decay_rate = pol->decay_rate; c->ac_decay_min = pol->decay_min;
    c->ac_update_method = ac->update_method[0] == 'p' ? 0 : 1;
    c->ac_step_limit = ac->step_limit.empty() ? -1. : ac->step_limit[0];
    c->table_log2_capacity = 16;                   // initial size: the tables grow between launches (grlx_config_cart_pole_ac)
    return;
  }

  // ---- discrete Q policies (cfg/pendulum/sarsa_tc.yaml, q_tc.yaml)
  const QPolicy *pol = dynamic_cast<const QPolicy *>(agent->policy);
  const TDPredictorBase *pred = dynamic_cast<const TDPredictorBase *>(agent->predictor);
  const QPolicy *tpol = test_agent ? dynamic_cast<const QPolicy *>(test_agent->policy) : nullptr;
  if (!pol || !pred || (test_agent && !tpol))
    throw Exception(path() + ": the accelerated path needs mapping/policy/discrete/value/q with predictor/critic/sarsa|q, or policy/action with predictor/ac/action");
  if (!pol->projector || !pol->representation || (tpol && (!tpol->projector || !tpol->representation)))
    throw Exception(path() + ": experiment/online_learning runs projector/tile_coding with representation/parameterized/linear on the accelerated path");
  if (pred->projector != pol->projector || pred->representation != pol->representation)
    throw Exception(pred->path() + ": predictor and policy must share projector and representation on the accelerated path");
  if (const ExpectedSARSAPredictor *es = dynamic_cast<const ExpectedSARSAPredictor *>(pred))
    if (es->target_policy != pol) throw Exception(es->path() + ": the target policy must be the agent's own policy on the accelerated path");
  if (tpol && (tpol->projector != pol->projector || tpol->representation != pol->representation || tpol->discretizer != pol->discretizer))
    throw Exception(test_agent->path() + ": the test policy must share discretizer, projector and representation with the learning policy");
  if (!pol->sampler->explores() || (tpol && tpol->sampler->explores()))
    throw Exception(path() + ": the accelerated path needs sampler/epsilon_greedy for learning and sampler/greedy for testing");
  // RNG streams are consumed in instantiate order: representation, learning sampler, test sampler
  const int at_repr = order_of(pol->representation), at_s1 = order_of(pol->sampler), at_s2 = tpol ? order_of(tpol->sampler) : -1;
  if (!(at_repr >= 0 && at_repr < at_s1 && (!tpol || at_s1 < at_s2)))
    throw Exception(path() + ": this yaml instantiates representation/samplers in an order the fused kernel does not reproduce");
  const UniformDiscretizer *d = pol->discretizer;
  if (d->min.size() != 1) throw Exception(d->path() + ": one action dimension supported");
  c->action_min = d->min[0]; c->action_max = d->max[0]; c->action_steps = (int)d->steps[0];
  pol->projector->lower(&c->projector);
  lower_linear(pol->representation, pol->projector, &c->representation);
  const EpsilonGreedySampler *sm = static_cast<const EpsilonGreedySampler *>(pol->sampler);
  c->epsilon = sm->epsilon[0]; c->decay_rate = sm->decay_rate; c->decay_min = sm->decay_min;
  c->agent = pred->agent_id();
  c->target_interval = pol->representation->interval;              // target network of the Q table (representation.h:161-306)
  c->target_tau = pol->representation->tau;
  c->alpha = pred->alpha; c->gamma = pred->gamma; c->lambda = pred->lambda; c->kappa = pred->kappa;
  c->trace = pred->trace ? pred->trace->kind() : GRLX_TRACE_NONE;
  if (const QVPredictor *qv = dynamic_cast<const QVPredictor *>(pred))
  { // second table: V(s); its weights are drawn from the thread-local stream after the Q table's
    if (!(order_of(qv->v_representation) > at_repr))
      throw Exception(qv->path() + ": v_representation must be instantiated after the policy's representation");
    qv->v_projector->lower(&c->actor_projector);
    lower_linear(qv->v_representation, qv->v_projector, &c->actor_representation);
    c->beta = qv->beta;
  }
}

// the parameterized representations of the agent in table order: 0 = Q / critic, 1 = actor / V
std::vector<const Configurable *> OnlineImpl::representations() const
{
  std::vector<const Configurable *> reprs;
  if (const ActionACPredictor *ac = dynamic_cast<const ActionACPredictor *>(agent->predictor))
  { reprs.push_back(ac->critic->representation); reprs.push_back(ac->representation); }
  else
  {
    reprs.push_back(dynamic_cast<const QPolicy *>(agent->policy)->representation);
    if (const QVPredictor *qv = dynamic_cast<const QVPredictor *>(agent->predictor)) reprs.push_back(qv->v_representation);
  }
  return reprs;
}

// ---- the experiment's objects stepped by the caller (StepwiseExperiment)
void ContextEnvironment::start(int test, const int32_t *active, double *obs) { check(grlx_env_start(ctx, test, active, obs), "environment/modeled: "); }
void ContextEnvironment::step(const int32_t *active, const double *action, double *obs, double *reward, int32_t *terminal)
{ check(grlx_env_advance(ctx, active, action, obs, reward, terminal), "environment/modeled: "); }
void ContextAgent::start(const int32_t *active, const double *obs, double *action) { check(grlx_agent_start(ctx, test, active, obs, action), "agent: "); }
void ContextAgent::step(const int32_t *active, double tau, const double *obs, const double *reward, const int32_t *terminal, double *action)
{ check(grlx_agent_step(ctx, test, active, tau, obs, reward, terminal, action), "agent: "); }
void ContextAgent::end(const int32_t *active, double tau, const double *obs, const double *reward)
{ check(grlx_agent_end(ctx, test, active, tau, obs, reward), "agent: "); }

void OnlineImpl::open(const RunOptions &opt)
{
  close();
  lower(&step_cfg);
  step_cfg.n_replicas = opt.replicas;
  if (opt.table_log2_capacity) step_cfg.table_log2_capacity = opt.table_log2_capacity;
  step_ctx = create_context(step_cfg, rules::clone_seeds(opt.seed, 0, opt.replicas).data());
  step_env.ctx = step_agent.ctx = step_test_agent.ctx = step_ctx.get();
  step_agent.test = 0;
  step_test_agent.test = 1;
}

// ---- run(): the plan stage.  Everything that is decided or refused before grlx_create; nothing here asks for a device.
RunPlan OnlineImpl::plan(const RunOptions &opt) const
{
  RunPlan p;
  p.opt = &opt;
  if (trials <= 0 && steps <= 0) throw Exception(path() + ": trials or steps must be > 0 (the reference's trials: 0, steps: 0 runs forever)");
  // the trial loop of online_learning.cpp:154 ends a run at the first trial boundary with `ss >= steps`, and save_every: test | trial
  // writes the policy between trials: both need the host between trials, so such runs launch one trial at a time
  p.by_trial = steps > 0 || save_every == "test" || save_every == "trial";
  if (steps > 0 && opt.replicas * opt.world > 1)
    throw Exception(path() + ": a steps budget ends every clone at a trial of its own; on the accelerated path it is built for one replica");
  p.trial_cap = rules::trial_cap(trials, steps, test_interval);
  grlx_config &c = p.c;
  lower(&c);
  c.n_replicas = opt.replicas;
  c.max_rows = rules::max_rows(p.trial_cap, test_interval);
  if (opt.table_log2_capacity) c.table_log2_capacity = opt.table_log2_capacity;
  // exact resume: -k reserves rows for a continuation; -K takes the snapshot's reservation, which the load compares
  p.snap_save = !opt.snapshot_save.empty();
  p.snap_load = !opt.snapshot_load.empty();
  if (p.snap_save || p.snap_load)
  {
    if (runs > 1) throw Exception(path() + ": a snapshot (-k / -K) is not built together with runs: " + std::to_string(runs) + " (one run per command)");
    if (steps > 0) throw Exception(path() + ": a snapshot (-k / -K) is not built together with a steps budget (steps: " + std::to_string(steps) + ")");
  }
  const int rows_needed = c.max_rows;
  c.max_rows = rules::reserved_rows(c.max_rows, p.snap_save);
  if (p.snap_load && !opt.plan_only)
  {
    grlx_snapshot_info_t snap_info;
    std::ifstream f(opt.snapshot_load, std::ios::binary | std::ios::ate);
    if (!f) throw Exception("-K: could not open the snapshot '" + opt.snapshot_load + "'");
    p.snapshot.resize((size_t)f.tellg());
    f.seekg(0);
    if (!f.read(p.snapshot.data(), (std::streamsize)p.snapshot.size())) throw Exception("-K: could not read the snapshot '" + opt.snapshot_load + "'");
    check(grlx_snapshot_info(p.snapshot.data(), p.snapshot.size(), &snap_info), "-K " + opt.snapshot_load + ": ");
    if (snap_info.trials_run > trials)
      throw Exception("-K " + opt.snapshot_load + ": the snapshot has run " + std::to_string(snap_info.trials_run) + " trials, this run asks for " + std::to_string(trials));
    if (snap_info.config.max_rows < rows_needed)
      throw Exception("-K " + opt.snapshot_load + ": the snapshot reserves " + std::to_string(snap_info.config.max_rows) + " test rows, " + std::to_string(trials) +
                      " trials need " + std::to_string(rows_needed));
    c.max_rows = snap_info.config.max_rows;
    p.first_trial = (int)snap_info.trials_run;
  }
  p.sweep = opt.sweep_repetitions > 0;
  p.group = p.sweep ? opt.sweep_repetitions : opt.replicas;
  p.query = !opt.query_file.empty();
  if (p.query)
  {
    if (opt.world > 1) throw Exception(path() + ": a policy query (-Q) runs on one GPU (-g " + std::to_string(opt.world) + " is not built)");
    if (c.agent == GRLX_AGENT_AC)
      throw Exception(path() + ": a policy query (-Q) is built for agents with a policy/discrete/q; ensemble statistics for the actor-critic are not built");
    if (p.group < 2) throw Exception(path() + ": -Q: -r must be >= 2: the standard deviation over the clones divides by n - 1");
    if (opt.query_cols != c.projector.dims - 1)
      throw Exception("-Q " + opt.query_file + ": " + std::to_string(opt.query_cols) + " columns, the agent's observation has " + std::to_string(c.projector.dims - 1));
    if (output.empty()) throw Exception(path() + ": -Q writes <output>-<run>-policy.txt: the experiment has no output");
  }
  if (opt.trajectory_steps != 0)
  { // -T rides on -E: refused here with its own name, before -E's checks say the same without it
    if (opt.evaluate_file.empty()) throw Exception(path() + ": -T: per-step trajectories need the start states of -E <states file>");
    if (opt.trajectory_steps < 1 || opt.trajectory_steps > GRLX_MAX_EPISODE_STEPS)
      throw Exception(path() + ": -T " + std::to_string(opt.trajectory_steps) + " is outside 1 ... GRLX_MAX_EPISODE_STEPS (" + std::to_string(GRLX_MAX_EPISODE_STEPS) + ")");
    if (opt.world > 1) throw Exception(path() + ": -T: trajectories of a policy evaluation run on one GPU (-g " + std::to_string(opt.world) + " is not built)");
    if (p.group < 2) throw Exception(path() + ": -T: -E needs -r >= 2: the standard deviation over the clones divides by n - 1");
  }
  if (opt.sampled_sampler >= 0)
  { // -e rides on -E: refused here with its own name, before -E's checks say the same without it
    if (opt.evaluate_file.empty()) throw Exception(path() + ": -e: a sampled evaluation needs the start states of -E <states file>");
    if (opt.world > 1) throw Exception(path() + ": -e: a sampled policy evaluation runs on one GPU (-g " + std::to_string(opt.world) + " is not built)");
    if (p.group < 2) throw Exception(path() + ": -e: -E needs -r >= 2: the standard deviation over the clones divides by n - 1");
    if (c.agent == GRLX_AGENT_AC)
      throw Exception(path() + ": -e: a sampled evaluation is not built for the actor-critic agent (its Gaussian / Ornstein-Uhlenbeck exploration needs the policy's noise state: -N <sigma | own> carries it)");
  }
  if (opt.noisy)
  { // -N rides on -E: refused here with its own name, before -E's checks say the same without it
    if (opt.evaluate_file.empty()) throw Exception(path() + ": -N: a noisy evaluation needs the start states of -E <states file>");
    if (opt.world > 1) throw Exception(path() + ": -N: a noisy policy evaluation runs on one GPU (-g " + std::to_string(opt.world) + " is not built)");
    if (p.sweep) throw Exception(path() + ": -N: a noisy evaluation is the actor-critic's, for which per-replica parameters (-p) are not built");
    if (p.group < 2) throw Exception(path() + ": -N: -E needs -r >= 2: the standard deviation over the clones divides by n - 1");
    if (c.agent != GRLX_AGENT_AC)
      throw Exception(path() + ": -N: a noisy evaluation serves the actor-critic agent only; the samplers of an agent with a policy/discrete/q are -e <epsilon | own | greedy>'s");
  }
  if (opt.actor_rule >= 0)
  { // -A rides on -E: refused here with its own name, before -E's checks say the same without it
    if (opt.evaluate_file.empty()) throw Exception(path() + ": -A: an actor ensemble's evaluation needs the start states of -E <states file>");
    if (opt.world > 1) throw Exception(path() + ": -A: an actor ensemble's evaluation runs on one GPU (-g " + std::to_string(opt.world) + " is not built)");
    if (p.sweep) throw Exception(path() + ": -A: an actor ensemble is the actor-critic's, for which per-replica parameters (-p) are not built");
    if (c.agent != GRLX_AGENT_AC)
      throw Exception(path() + ": -A: an actor ensemble serves the actor-critic agent only; the vote and the mean Q of an agent with a policy/discrete/q are -V <vote | mean>'s");
  }
  p.evaluate = !opt.evaluate_file.empty();
  if (p.evaluate)
  { // (grlx_evaluate validates the states themselves, and what it is built for, before it launches)
    if (opt.world > 1) throw Exception(path() + ": a policy evaluation (-E) runs on one GPU (-g " + std::to_string(opt.world) + " is not built)");
    if (p.group < 2) throw Exception(path() + ": -E: -r must be >= 2: the standard deviation over the clones divides by n - 1");
    int state_dims = 0;
    check(grlx_env_dims(c.env, &state_dims, nullptr), path() + ": -E: ");
    if (opt.evaluate_cols != state_dims)
      throw Exception("-E " + opt.evaluate_file + ": " + std::to_string(opt.evaluate_cols) + " columns, the model's state has " + std::to_string(state_dims) +
                      " (the time included)");
    if (output.empty()) throw Exception(path() + ": -E writes <output>-<run>-returns.txt: the experiment has no output");
    if (opt.ensemble_rule >= 0 && c.agent == GRLX_AGENT_AC)
      throw Exception(path() + ": -V: an ensemble evaluation is not built for the actor-critic agent (a vote over continuous actions is mapping/policy/multi's: -A <rule> combines them)");
  }
  if (p.sweep)
  {
    if (steps > 0) throw Exception(path() + ": a parameter sweep (-p) is not built together with a steps budget (steps: " + std::to_string(steps) + ")");
    if (opt.world > 1) throw Exception(path() + ": a parameter sweep (-p) runs on one GPU (-g " + std::to_string(opt.world) + " is not built)");
    for (int k = 0; k < 4; ++k)
      if (!opt.sweep[k].empty() && (int)opt.sweep[k].size() != opt.replicas) throw Exception(path() + ": a sweep needs one value per clone");
  }
  p.first_clone = opt.rank * opt.replicas;
  p.many = opt.replicas * opt.world > 1;
  if (opt.plan_only) return p;                       // -n prints the clones and runs nothing: no log, no taps
  grlx_env_dims(c.env, &p.state_dims, &p.obs_dims);
  if (exporter || env_exporter)
  { // transition log of replica 0: every step and every trial start is tapped on the device and
    // written after the run (the reference writes one row per step, online_learning.cpp:183-206)
    const double per_trial = std::floor(c.timeout / c.control_step) + 3;
    const double want = per_trial * (double)p.trial_cap;
    if (want > 4e6) throw Exception(path() + ": transition log of " + std::to_string((long long)want) + " rows is too large for the device-side tap buffer");
    c.tap_replica = 0;
    c.tap_capacity = (int)want;
    c.tap_starts = 1;
  }
  return p;
}

// -n: one line per clone of this process: i seed alpha gamma lambda epsilon
void OnlineImpl::print_plan(const RunPlan &p) const
{
  const RunOptions &opt = *p.opt;
  const double shared[4] = {p.c.alpha, p.c.gamma, p.c.lambda, p.c.epsilon};
  for (int i = 0; i < opt.replicas; ++i)
  {
    char line[256];
    int at = snprintf(line, sizeof(line), "%d %lld", p.first_clone + i, (long long)(opt.seed + p.first_clone + i));
    for (int k = 0; k < 4; ++k) at += snprintf(line + at, sizeof(line) - (size_t)at, " %.17g", rules::sweep_value(opt.sweep[k], shared[k], (size_t)i));
    std::cout << line << std::endl;
  }
}

// grlx_set_replica_params validates one parameter against the other three as they stand.  So that a grid whose final (gamma, lambda)
// pairs are all valid is never refused on the way there, lambda first goes to min(the yaml's, the grid's) -- a shorter trace is
// always valid --, then gamma, then lambda.
void OnlineImpl::apply_sweep(const RunPlan &p, grlx_ctx *ctx) const
{
  if (!p.sweep) return;
  const RunOptions &opt = *p.opt;
  std::vector<std::pair<int, const double *>> calls;
  std::vector<double> lambda_low;
  if (!opt.sweep[GRLX_PARAM_GAMMA].empty() && !opt.sweep[GRLX_PARAM_LAMBDA].empty())
  {
    for (double v : opt.sweep[GRLX_PARAM_LAMBDA]) lambda_low.push_back(v < p.c.lambda ? v : p.c.lambda);
    calls.push_back({GRLX_PARAM_LAMBDA, lambda_low.data()});
  }
  for (int k = 0; k < 4; ++k)
    if (!opt.sweep[k].empty()) calls.push_back({k, opt.sweep[k].data()});
  for (const auto &call : calls) check(grlx_set_replica_params(ctx, call.first, call.second));
}

void OnlineImpl::load_snapshot(RunPlan &p, grlx_ctx *ctx) const
{
  if (!p.snap_load) return;
  check(grlx_snapshot_load(ctx, p.snapshot.data(), p.snapshot.size()), "-K " + p.opt->snapshot_load + ": ");
  std::vector<char>().swap(p.snapshot);
}

// Load policy every run (online_learning.cpp:140-150 -> ParameterizedRepresentation {action: load},
// representation.h:231-263): <load_file with $run -> run>-<config path with '/'->'_'>.dat, raw
// double[memory]; a missing or wrong-sized file is a warning, not an error, as in the reference.
// All clones of a run read the same file (multi.cpp does not touch load_file).
void OnlineImpl::load_policy(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  if (load_file.empty()) return;
  std::string base = load_file;
  for (size_t at; (at = base.find("$run")) != std::string::npos;) base.replace(at, 4, std::to_string(run));
  log(2, "Loading policy: " + base + "-");
  const std::vector<const Configurable *> reprs = representations();
  for (size_t tb = 0; tb < reprs.size(); ++tb)
  {
    const std::string file = rules::dat_name(base, false, 0, reprs[tb]->path());
    const size_t memory = (size_t)rules::table_memory(p.c, (int)tb);
    std::ifstream f(file, std::ios::binary | std::ios::ate);
    if (!f) { log(1, "Could not open '" + file + "' for reading"); continue; }
    if ((size_t)f.tellg() != memory * sizeof(double)) { log(1, "Configuration mismatch for '" + file + "'"); continue; }
    std::vector<double> dense(memory);
    f.seekg(0);
    if (!f.read(reinterpret_cast<char *>(dense.data()), (std::streamsize)(memory * sizeof(double)))) { log(1, "Could not read '" + file + "'"); continue; }
    check(grlx_load_weights(ctx, (int)tb, 0, p.opt->replicas, dense.data(), (uint64_t)memory));
  }
}

// ParameterizedRepresentation {action: save} (representation.h:201-229) of every representation of the agent: raw double[memory] to
// the file rules::dat_name gives <base> (online_learning.cpp:281-302: <output>-run<run>[-trial<tt>])
void OnlineImpl::save_policy(const RunPlan &p, grlx_ctx *ctx, const std::string &base) const
{
  const int replicas = p.opt->replicas;
  const std::vector<const Configurable *> reprs = representations();
  for (size_t tb = 0; tb < reprs.size(); ++tb)
    for (int i = 0; i < replicas; ++i)
    {
      std::vector<double> dense((size_t)rules::table_memory(p.c, (int)tb));
      check(grlx_export_weights(ctx, (int)tb, i, dense.data()));
      const std::string name = rules::dat_name(base, replicas > 1, i, reprs[tb]->path());
      std::ofstream f(name, std::ios::binary);
      if (!f) { log(1, "Could not open '" + name + "' for writing"); continue; }
      f.write(reinterpret_cast<const char *>(dense.data()), (std::streamsize)(dense.size() * sizeof(double)));
    }
}

// one launch for the whole run, or -- a steps budget, save_every: test | trial -- one per trial with the host in between
void OnlineImpl::trial_loop(const RunPlan &p, grlx_ctx *ctx, int run) const
{
  if (!p.by_trial)
  {
    check(grlx_run(ctx, trials - p.first_trial, nullptr));
    check(grlx_sync(ctx, nullptr));
    return;
  }
  // for (ss = 0, tt = 0; (!trials || tt < trials) && (!steps || ss < steps); ++tt)   -- online_learning.cpp:154
  uint64_t learn0 = 0, test0 = 0;
  grlx_step_counts(ctx, &learn0, &test0);
  uint64_t ss = 0;
  for (int tt = p.first_trial; (trials <= 0 || tt < trials) && (steps <= 0 || ss < (uint64_t)steps); ++tt)
  {
    check(grlx_run(ctx, 1, nullptr));
    check(grlx_sync(ctx, nullptr));
    uint64_t learn = 0, test = 0;
    grlx_step_counts(ctx, &learn, &test);
    ss = learn - learn0;                         // one replica when a budget is set; unused otherwise
    const bool was_test = test_interval >= 0 && tt % (test_interval + 1) == test_interval;
    if ((save_every == "trial" || (was_test && save_every == "test")) && !output.empty())
      save_policy(p, ctx, output + "-run" + std::to_string(run) + "-trial" + std::to_string(tt));      // online_learning.cpp:281-290
  }
}

// -k: the whole context, as it stands at the end of the trial loop
void OnlineImpl::save_snapshot(const RunPlan &p, grlx_ctx *ctx) const
{
  if (!p.snap_save) return;
  const std::string &file = p.opt->snapshot_save;
  uint64_t bytes = 0, written = 0;
  check(grlx_snapshot_size(ctx, &bytes), "-k " + file + ": ");
  std::vector<char> buf((size_t)bytes);
  check(grlx_snapshot_save(ctx, buf.data(), bytes, &written), "-k " + file + ": ");
  std::ofstream f(file, std::ios::binary | std::ios::trunc);
  if (!f.write(buf.data(), (std::streamsize)written) || !f.flush()) throw Exception("-k: could not write the snapshot '" + file + "'");
}

// the transition log of replica 0, in device order; empty without an exporter
std::vector<grlx_tap> OnlineImpl::read_taps(const RunPlan &p, grlx_ctx *ctx) const
{
  std::vector<grlx_tap> taps;
  if (!exporter && !env_exporter) return taps;
  int ntaps = 0;
  taps.resize((size_t)p.c.tap_capacity);
  check(grlx_read_taps(ctx, taps.data(), p.c.tap_capacity, &ntaps));
  if (ntaps == p.c.tap_capacity) log(1, "transition log truncated at " + std::to_string(ntaps) + " rows");
  taps.resize((size_t)ntaps);
  return taps;
}

std::vector<double> OnlineImpl::run(const RunOptions &opt)
{
  RunPlan p = plan(opt);
  std::vector<double> curve;
  if (opt.plan_only) { print_plan(p); return curve; }
  if (!output.empty())
  { // store the resolved configuration with the output (online_learning.cpp:117-122)
    std::ofstream ofs(output + ".yaml");
    ofs << configurator->root()->yaml();
  }
  // ONE instantiation for all runs, as in the reference: between two runs the experiment is reset (online_learning.cpp:307-308),
  // not re-created -- the random streams continue, so run 1 differs from a fresh process with another seed
  const CtxOwner owner = create_context(p.c, rules::clone_seeds(opt.seed, p.first_clone, opt.replicas).data());
  grlx_ctx *ctx = owner.get();
  apply_sweep(p, ctx);
  load_snapshot(p, ctx);
  for (int rr = run_offset; rr < runs + run_offset; ++rr)
  {
    load_policy(p, ctx, rr);
    RunRows rows;
    const auto start = std::chrono::steady_clock::now();
    trial_loop(p, ctx, rr);
    save_snapshot(p, ctx);
    rows.wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();

    const std::vector<grlx_tap> taps = read_taps(p, ctx);
    if (env_exporter) write_environment_log(env_exporter, taps, p.state_dims, p.obs_dims, p.c.control_step);
    if (exporter) write_experiment_log(exporter, taps, p.obs_dims);

    write_rows(p, ctx, rr, &rows, &curve);
    write_sweep_file(p, rr, rows);
    write_policy_file(p, ctx, rr);
    write_returns_file(p, ctx, rr);
    write_ensemble_file(p, ctx, rr);
    write_trajectory_files(p, ctx, rr);
    write_sampled_files(p, ctx, rr);
    write_noisy_files(p, ctx, rr);
    write_actor_ensemble_files(p, ctx, rr);
    write_mean_file(p, ctx, rr, rows);
    if (save_every == "run" && !output.empty()) save_policy(p, ctx, output + "-run" + std::to_string(rr));      // online_learning.cpp:294-302

    uint64_t learn = 0, test = 0;
    grlx_step_counts(ctx, &learn, &test);
    std::ostringstream msg;
    msg << "run " << rr << ": " << opt.replicas << " replicas, " << (learn + test) << " env-steps in " << rows.wall << " s = "
        << (double)(learn + test) / rows.wall / 1e6 << " M env-steps/s";
    log(2, msg.str());
    if (rr < runs + run_offset - 1) check(grlx_reset_run(ctx));        // online_learning.cpp:307-308
  }
  return curve;
}
GRLX_REGISTER(OnlineLearningExperimentImpl)

} // namespace grlx_host
