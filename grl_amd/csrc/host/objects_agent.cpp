// objects_agent.cpp -- the agent side of the graph: discretizer, projector, representation, samplers, policies, traces, predictors
// and agents (declared in objects_impl.h).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "objects_impl.h"

namespace grlx_host {

// discretizer/uniform (uniform.cpp:34-95)
void UniformDiscretizer::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("min", "Lower limit", VecD{}, CRP::System));
  config->push_back(CRP("max", "Upper limit", VecD{}, CRP::System));
  config->push_back(CRP("steps", "Discretization steps per dimension", VecD{}));
}
void UniformDiscretizer::configure(Configuration &config)
{
  min = config["min"].v(); max = config["max"].v(); steps = config["steps"].v();
  if (min.size() != max.size() || min.size() != steps.size()) throw bad_param("discretizer/uniform:{min,max,steps}");
  for (double s : steps) if (s < 1) throw bad_param("discretizer/uniform:steps");
}
GRLX_REGISTER(UniformDiscretizer)

// projector/tile_coding (tile_coding.cpp:34-80)
void TileCodingProjector::lower(grlx_tile_spec *t) const
{
  memset(t, 0, sizeof(*t));
  t->tilings = tilings; t->memory = memory; t->dims = (int)resolution.size();
  t->safe = safe;
  if (resolution.size() > GRLX_MAX_DIMS) throw bad_param("projector/tile_coding:resolution");
  for (size_t i = 0; i < resolution.size(); ++i) { t->resolution[i] = resolution[i]; t->wrapping[i] = wrapping[i]; }
}
void TileCodingProjector::project(const double *in, int n, uint32_t *out) const
{ // TileCodingProjector::_project for n inputs, on the GPU
  grlx_tile_spec t;
  lower(&t);
  // safe >= 1 returns CLAIMED slots, which depend on what was written before (tile_coding.h:116-151): that state lives in an
  // experiment's tables, not in a stand-alone projector -- refuse rather than return the unclaimed `hash % memory`
  if (safe != 0) throw Exception(path() + ": Projector::project as a stand-alone operator serves safe = 0 only (claims live in the experiment's tables)");
  check(grlx_project(&t, in, n, out), path() + ": ");
}
void TileCodingProjector::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("tilings", "Number of tilings", 16));
  config->push_back(CRP("memory", "Hash table size", 8 * 1024 * 1024));
  config->push_back(CRP("safe", "Collision detection (0=off, 1=claim on write, 2=claim always)", 0));
  config->push_back(CRP("resolution", "Size of a single tile", VecD{}));
  config->push_back(CRP("wrapping", "Wrapping boundaries (must be multiple of resolution)", VecD{}));
}
void TileCodingProjector::configure(Configuration &config)
{
  tilings = config["tilings"]; memory = config["memory"]; safe = config["safe"];
  resolution = config["resolution"].v(); wrapping = config["wrapping"].v();
  if (wrapping.empty()) wrapping.assign(resolution.size(), 0.);
  if (wrapping.size() != resolution.size()) throw bad_param("projector/tile_coding:wrapping");
  for (size_t ii = 0; ii < resolution.size(); ++ii)
  { // tile_coding.cpp:66-78
    double w = wrapping[ii] * (tilings / resolution[ii]);
    if (std::fabs(w - std::round(w)) > 0.001) throw bad_param("projector/tile_coding:wrapping");
  }
  if (safe < 0 || safe > 2) throw Exception(path() + ": safe must be 0, 1 or 2");
}
GRLX_REGISTER(TileCodingProjector)

// representation/parameterized/linear (linear.cpp:34-101)
void LinearRepresentation::reset(int64_t seed)
{
  if (outputs != 1) throw Exception(path() + ": the GPU operators serve representations with one output");
  // a representation with a target network (interval) reads through target() and counts updates towards the next
  // synchronisation (representation.h:266-306): the stand-alone operators do not carry that state -- refuse
  if (interval != 0) throw Exception(path() + ": Representation::read/write/update as stand-alone operators serve interval = 0 only (no target network)");
  own = nullptr;                                        // the old parameters go before the new ones are drawn
  grlx_config c;
  grlx_config_pendulum_sarsa(&c);
  c.n_replicas = 1;
  c.projector.memory = memory;
  c.representation.init_min = init_min[0];
  c.representation.init_max = init_max[0];
  c.representation.output_min = output_min[0];
  c.representation.output_max = output_max[0];
  c.representation.limit = limit;
  own = create_context(c, &seed, path() + ": ");
}
grlx_ctx *LinearRepresentation::context()
{
  if (!own) reset(1);
  return own.get();
}
void LinearRepresentation::read(const uint32_t *idx, int n, double *out)
{
  const std::vector<int32_t> rep((size_t)n, 0);
  check(grlx_read(context(), 0, rep.data(), idx, n, out), path() + ": ");
}
void LinearRepresentation::write(const uint32_t *idx, int n, const double *target, double alpha)
{
  const std::vector<int32_t> rep((size_t)n, 0);
  check(grlx_write(context(), 0, rep.data(), idx, n, target, alpha), path() + ": ");
}
void LinearRepresentation::update(const uint32_t *idx, int n, const double *delta)
{
  const std::vector<int32_t> rep((size_t)n, 0);
  check(grlx_update(context(), 0, rep.data(), idx, n, delta), path() + ": ");
}
void LinearRepresentation::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("init_min", "Lower initial value limit", VecD{0.}));
  config->push_back(CRP("init_max", "Upper initial value limit", VecD{1.}));
  config->push_back(CRP("memory", "Feature vector size", 8 * 1024 * 1024, CRP::System));
  config->push_back(CRP("outputs", "Number of outputs", 1, CRP::System));
  config->push_back(CRP("output_min", "Lower output limit", VecD{}, CRP::System));
  config->push_back(CRP("output_max", "Upper output limit", VecD{}, CRP::System));
  config->push_back(CRP("limit", "Limit parameters to same range as outputs", 1));
  config->push_back(CRP("interval", "Target network update interval", 0.));     // ParameterizedRepresentation (unused here)
  config->push_back(CRP("tau", "Target network update rate", 1.));
}
void LinearRepresentation::configure(Configuration &config)
{
  memory = config["memory"]; outputs = config["outputs"]; limit = config["limit"];
  init_min = config["init_min"].v(); init_max = config["init_max"].v();
  if (!init_min.empty() && (int)init_min.size() < outputs) init_min.assign((size_t)outputs, init_min[0]);
  if ((int)init_min.size() != outputs) throw bad_param("representation/parameterized/linear:init_min");
  if (!init_max.empty() && (int)init_max.size() < outputs) init_max.assign((size_t)outputs, init_max[0]);
  if ((int)init_max.size() != outputs) throw bad_param("representation/parameterized/linear:max");
  output_min = config["output_min"].v();
  if (output_min.empty()) output_min.assign((size_t)outputs, -DBL_MAX);
  if ((int)output_min.size() != outputs) throw bad_param("representation/parameterized/linear:output_min");
  output_max = config["output_max"].v();
  if (output_max.empty()) output_max.assign((size_t)outputs, DBL_MAX);
  if ((int)output_max.size() != outputs) throw bad_param("representation/parameterized/linear:output_max");
  interval = (int)(double)config["interval"];                   // ParameterizedRepresentation (representation.h:173-190)
  tau = config["tau"];
  if (interval < 0 || !(tau >= 0 && tau <= 1)) throw bad_param("representation/parameterized/linear:{interval,tau}");
}
GRLX_REGISTER(LinearRepresentation)

// sampler/greedy, sampler/epsilon_greedy (greedy.cpp:34-130)
GRLX_REGISTER(GreedySampler)
void EpsilonGreedySampler::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("epsilon", "Exploration rate (can be defined per action)", VecD{0.05}, CRP::Online));
  config->push_back(CRP("decay_rate", "Multiplicative decay factor per episode", 1.));
  config->push_back(CRP("decay_min", "Minimum decay (eps_min = eps*decay_min)", 0.));
}
void EpsilonGreedySampler::configure(Configuration &config)
{
  epsilon = config["epsilon"].v(); decay_rate = config["decay_rate"]; decay_min = config["decay_min"];
  if (epsilon.size() < 1) throw bad_param("sampler/epsilon_greedy:epsilon");
  if (epsilon.size() > 1) throw Exception(path() + ": per-action epsilon is outside the accelerated path");
}
GRLX_REGISTER(EpsilonGreedySampler)

// mapping/policy/action (action.cpp:38-91)
void ActionPolicy::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("sigma", "Standard deviation of Gaussian exploration distribution", VecD{}));
  config->push_back(CRP("theta", "Ornstein-Uhlenbeck friction term (1=pure Gaussian noise)", VecD{}));
  config->push_back(CRP("decay_rate", "Multiplicative decay factor per episode", 1.));
  config->push_back(CRP("decay_min", "Minimum decay (sigma_min = sigma*decay_min)", 0.));
  config->push_back(CRP("renormalize", "Renormalize representation output from [-1, 1] to [min, max]", 0));
  config->push_back(CRP("output_min", "Lower limit on outputs", VecD{}, CRP::System));
  config->push_back(CRP("output_max", "Upper limit on outputs", VecD{}, CRP::System));
  config->push_back(CRP("projector", "projector.observation", "Projects observations onto representation space", (Configurable *)nullptr));
  config->push_back(CRP("representation", "representation.action", "Action representation", (Configurable *)nullptr));
}
void ActionPolicy::configure(Configuration &config)
{
  projector = dynamic_cast<TileCodingProjector *>(config["projector"].ptr());
  representation = dynamic_cast<LinearRepresentation *>(config["representation"].ptr());
  sigma = config["sigma"].v(); theta = config["theta"].v();
  decay_rate = config["decay_rate"]; decay_min = config["decay_min"];
  min = config["output_min"].v(); max = config["output_max"].v();
  if (min.size() != max.size() || min.empty()) throw bad_param("policy/action:{output_min,output_max}");
  if (sigma.empty()) sigma = VecD{0.};
  if (sigma.size() == 1) sigma.assign(min.size(), sigma[0]);
  if (sigma.size() != min.size()) throw bad_param("policy/action:sigma");
  if (theta.empty()) theta = VecD{1.};
  if (theta.size() == 1) theta.assign(min.size(), theta[0]);
  if (theta.size() != min.size()) throw bad_param("policy/action:theta");
  if ((int)config["renormalize"] != 0) throw Exception(path() + ": renormalize is outside the accelerated path");
  if (!projector || !representation) throw Exception(path() + ": projector/representation outside the accelerated path");
  if (min.size() != 1) throw Exception(path() + ": one action dimension supported");
}
GRLX_REGISTER(ActionPolicy)

// mapping/policy/discrete/value/q (q.cpp:35-52)
void QPolicy::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("discretizer", "discretizer.action", "Action discretizer", (Configurable *)nullptr));
  config->push_back(CRP("projector", "projector.pair", "Projects observation-action pairs onto representation space", (Configurable *)nullptr));
  config->push_back(CRP("representation", "representation.value/action", "Action-value representation", (Configurable *)nullptr));
  config->push_back(CRP("sampler", "sampler", "Samples actions from action-values", (Configurable *)nullptr));
}
void QPolicy::configure(Configuration &config)
{
  discretizer = dynamic_cast<UniformDiscretizer *>(config["discretizer"].ptr());
  projector = dynamic_cast<TileCodingProjector *>(config["projector"].ptr());
  representation = dynamic_cast<LinearRepresentation *>(config["representation"].ptr());
  sampler = dynamic_cast<GreedySampler *>(config["sampler"].ptr());
  any_projector = config["projector"].ptr();
  any_representation = config["representation"].ptr();
  // (projector / representation kinds are checked where the graph is lowered: tile coding + linear for experiment/online_learning,
  //  projector/pre/normalizing + representation/iterative over an ANN for experiment/batch_learning)
  if (!discretizer || !any_projector || !any_representation || !sampler)
    throw Exception(path() + ": the accelerated path needs discretizer/uniform, a projector, a representation and a greedy sampler");
}
GRLX_REGISTER(QPolicy)
struct QPolicyLegacy : QPolicy { GRLX_TYPEINFO("mapping/policy/discrete/q") };      // name used by tests/pendulum-sarsa-tc.yaml
GRLX_REGISTER(QPolicyLegacy)

struct ReplacingTrace : Trace { GRLX_TYPEINFO("trace/enumerated/replacing") int kind() const override { return GRLX_TRACE_REPLACING; } };
GRLX_REGISTER(ReplacingTrace)
struct AccumulatingTrace : Trace { GRLX_TYPEINFO("trace/enumerated/accumulating") int kind() const override { return GRLX_TRACE_ACCUMULATING; } };
GRLX_REGISTER(AccumulatingTrace)

// what every predictor takes besides its own parameters (Predictor::request)
static void request_importer_exporter(ConfigurationRequest *config)
{
  config->push_back(CRP("importer", "importer", "Optional importer", (Configurable *)nullptr, true));
  config->push_back(CRP("exporter", "exporter", "Optional exporter", (Configurable *)nullptr, true));
}

// predictor/critic/sarsa (sarsa.cpp:35-60), predictor/critic/q (advantage.cpp:35-62)
void TDPredictorBase::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("alpha", "Learning rate", 0.2));
  config->push_back(CRP("gamma", "Discount rate", 0.97));
  config->push_back(CRP("lambda", "Trace decay rate", 0.65));
  if (agent_id() == GRLX_AGENT_ADVANTAGE)
    config->push_back(CRP("kappa", "Advantage scaling factor", 0.2));          // advantage.cpp:188
  if (agent_id() == GRLX_AGENT_Q || agent_id() == GRLX_AGENT_ADVANTAGE)
    config->push_back(CRP("discretizer", "discretizer.action", "Action discretizer", (Configurable *)nullptr));
  config->push_back(CRP("projector", "projector.pair", "Projects observation-action pairs onto representation space", (Configurable *)nullptr));
  config->push_back(CRP("representation", "representation.value/action", "Q-value representation", (Configurable *)nullptr));
  config->push_back(CRP("trace", "trace", "Trace of projections", (Configurable *)nullptr, true));
  request_importer_exporter(config);
}
void TDPredictorBase::configure(Configuration &config)
{
  alpha = config["alpha"]; gamma = config["gamma"]; lambda = config["lambda"];
  if (agent_id() == GRLX_AGENT_ADVANTAGE) kappa = config["kappa"];
  projector = dynamic_cast<TileCodingProjector *>(config["projector"].ptr());
  representation = dynamic_cast<LinearRepresentation *>(config["representation"].ptr());
  trace = dynamic_cast<Trace *>(config["trace"].ptr());
  if (!projector || !representation) throw Exception(path() + ": projector/representation outside the accelerated path");
  if (config["importer"].ptr() || config["exporter"].ptr()) throw Exception(path() + ": importer/exporter are outside the accelerated path");
}
struct SARSAPredictor : TDPredictorBase { GRLX_TYPEINFO("predictor/critic/sarsa") int agent_id() const override { return GRLX_AGENT_SARSA; } };
GRLX_REGISTER(SARSAPredictor)
struct QPredictor : TDPredictorBase { GRLX_TYPEINFO("predictor/critic/q") int agent_id() const override { return GRLX_AGENT_Q; } };
GRLX_REGISTER(QPredictor)
// predictor/critic/advantage (advantage.cpp:181-268): advantage learning, scaling factor kappa
struct AdvantagePredictor : TDPredictorBase { GRLX_TYPEINFO("predictor/critic/advantage") int agent_id() const override { return GRLX_AGENT_ADVANTAGE; } };
GRLX_REGISTER(AdvantagePredictor)
// predictor/critic/expected_sarsa (sarsa.cpp:134-165)
void ExpectedSARSAPredictor::request(const std::string &role, ConfigurationRequest *config)
{
  TDPredictorBase::request(role, config);
  config->push_back(CRP("policy", "mapping/policy/discrete/value", "Value based target policy", (Configurable *)nullptr));
}
void ExpectedSARSAPredictor::configure(Configuration &config)
{
  TDPredictorBase::configure(config);
  target_policy = config["policy"].ptr();
}
GRLX_REGISTER(ExpectedSARSAPredictor)
// predictor/critic/qv (qv.cpp:35-64)
void QVPredictor::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("alpha", "State-action value learning rate", 0.2));
  config->push_back(CRP("beta", "State value learning rate", 0.1));
  config->push_back(CRP("gamma", "Discount rate", 0.97));
  config->push_back(CRP("lambda", "Trace decay rate", 0.65));
  config->push_back(CRP("q_projector", "projector.pair", "Projects observation-action pairs onto representation space", (Configurable *)nullptr));
  config->push_back(CRP("q_representation", "representation.value/action", "State-action value representation (Q)", (Configurable *)nullptr));
  config->push_back(CRP("v_projector", "projector.observation", "Projects observations onto representation space", (Configurable *)nullptr));
  config->push_back(CRP("v_representation", "representation.value/state", "State value representation (V)", (Configurable *)nullptr));
  config->push_back(CRP("trace", "trace", "Trace of projections", (Configurable *)nullptr, true));
  request_importer_exporter(config);
}
void QVPredictor::configure(Configuration &config)
{
  alpha = config["alpha"]; beta = config["beta"]; gamma = config["gamma"]; lambda = config["lambda"];
  projector = dynamic_cast<TileCodingProjector *>(config["q_projector"].ptr());
  representation = dynamic_cast<LinearRepresentation *>(config["q_representation"].ptr());
  v_projector = dynamic_cast<TileCodingProjector *>(config["v_projector"].ptr());
  v_representation = dynamic_cast<LinearRepresentation *>(config["v_representation"].ptr());
  trace = dynamic_cast<Trace *>(config["trace"].ptr());
  if (!projector || !representation || !v_projector || !v_representation) throw Exception(path() + ": projectors/representations outside the accelerated path");
  if (config["importer"].ptr() || config["exporter"].ptr()) throw Exception(path() + ": importer/exporter are outside the accelerated path");
}
GRLX_REGISTER(QVPredictor)
// names from before the reference's predictor/critic/* rename, still used by its tests/pendulum-sarsa-tc.yaml
struct SARSAPredictorLegacy : SARSAPredictor { GRLX_TYPEINFO("predictor/sarsa") };
GRLX_REGISTER(SARSAPredictorLegacy)
struct QPredictorLegacy : QPredictor { GRLX_TYPEINFO("predictor/q") };
GRLX_REGISTER(QPredictorLegacy)

// predictor/critic/td (predictors/td.cpp:35-58): V(s) critic with a trace
void VPredictor::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("alpha", "Learning rate", 0.2));
  config->push_back(CRP("gamma", "Discount rate", 0.97));
  config->push_back(CRP("lambda", "Trace decay rate", 0.65));
  config->push_back(CRP("projector", "projector.observation", "Projects observations onto representation space", (Configurable *)nullptr));
  config->push_back(CRP("representation", "representation.value/state", "State value representation", (Configurable *)nullptr));
  config->push_back(CRP("trace", "trace", "Trace of projections", (Configurable *)nullptr, true));
  request_importer_exporter(config);
}
void VPredictor::configure(Configuration &config)
{
  alpha = config["alpha"]; gamma = config["gamma"]; lambda = config["lambda"];
  projector = dynamic_cast<TileCodingProjector *>(config["projector"].ptr());
  representation = dynamic_cast<LinearRepresentation *>(config["representation"].ptr());
  trace = dynamic_cast<Trace *>(config["trace"].ptr());
  if (!projector || !representation) throw Exception(path() + ": projector/representation outside the accelerated path");
  if (config["importer"].ptr() || config["exporter"].ptr()) throw Exception(path() + ": importer/exporter are outside the accelerated path");
}
GRLX_REGISTER(VPredictor)

// predictor/ac/action (ac.cpp:36-70)
void ActionACPredictor::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("alpha", "Critic learning rate", 0.01));
  config->push_back(CRP("update_method", "Actor update method", std::string("proportional")));
  config->push_back(CRP("step_limit", "Actor exploration step limit", VecD{}));
  config->push_back(CRP("projector", "projector.observation", "Projects observations onto actor representation space", (Configurable *)nullptr));
  config->push_back(CRP("representation", "representation.action", "Action representation", (Configurable *)nullptr));
  config->push_back(CRP("critic", "predictor/critic", "Critic predictor", (Configurable *)nullptr));
  request_importer_exporter(config);
}
void ActionACPredictor::configure(Configuration &config)
{
  alpha = config["alpha"]; update_method = config["update_method"].str(); step_limit = config["step_limit"].v();
  projector = dynamic_cast<TileCodingProjector *>(config["projector"].ptr());
  representation = dynamic_cast<LinearRepresentation *>(config["representation"].ptr());
  critic = dynamic_cast<VPredictor *>(config["critic"].ptr());
  if (update_method != "proportional" && update_method != "cacla") throw bad_param("predictor/ac/action:update_method");
  if (step_limit.size() > 1) throw bad_param("predictor/ac:step_limit");
  if (!projector || !representation || !critic) throw Exception(path() + ": the accelerated path needs tile coding, a linear actor and a predictor/critic/td critic");
}
GRLX_REGISTER(ActionACPredictor)

// agent/td (td.cpp:34-48), agent/fixed (fixed.cpp:34-45)
void TDAgent::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("policy", "mapping/policy", "Control policy", (Configurable *)nullptr));
  config->push_back(CRP("predictor", "predictor", "Value function predictor", (Configurable *)nullptr));
}
void TDAgent::configure(Configuration &config)
{
  policy = dynamic_cast<Policy *>(config["policy"].ptr());
  predictor = dynamic_cast<Predictor *>(config["predictor"].ptr());
  if (!policy || !predictor) throw Exception(path() + ": policy/predictor outside the accelerated path");
}
GRLX_REGISTER(TDAgent)
void FixedAgent::request(const std::string &, ConfigurationRequest *config)
{ config->push_back(CRP("policy", "mapping/policy", "Control policy", (Configurable *)nullptr)); }
void FixedAgent::configure(Configuration &config)
{
  policy = dynamic_cast<Policy *>(config["policy"].ptr());
  if (!policy) throw Exception(path() + ": policy outside the accelerated path");
}
GRLX_REGISTER(FixedAgent)

} // namespace grlx_host
