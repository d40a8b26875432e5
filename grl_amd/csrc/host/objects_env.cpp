// objects_env.cpp -- the environment side of the graph: dynamics, tasks, models, environment/modeled and its lowering to the
// environment fields of a grlx_config.
#include <cmath>

#include "objects_impl.h"

namespace grlx_host {

// the limits a task provides, under the names environment/modeled forwards
static void provide_task_outputs(ConfigurationRequest *config, const char *what)
{
  for (const char *n : rules::kTaskOutputs) config->push_back(CRP::provided(n, std::string("vector.") + n, what));
}

// dynamics/pendulum (pendulum.cpp:36-49): no parameters
struct PendulumDynamics : Dynamics {
  GRLX_TYPEINFO("dynamics/pendulum")
  int env_id() const override { return GRLX_ENV_PENDULUM; }
};
GRLX_REGISTER(PendulumDynamics)

// task/pendulum/swingup (pendulum.cpp:70-95)
struct PendulumSwingupTask : Task {
  GRLX_TYPEINFO("task/pendulum/swingup")
  int env_id() const override { return GRLX_ENV_PENDULUM; }
  void request(const std::string &, ConfigurationRequest *config) override
  {
    config->push_back(CRP("timeout", "Episode timeout", 2.99));
    config->push_back(CRP("randomization", "Level of start state randomization", 0.));
    config->push_back(CRP::provided("observation_dims", "int.observation_dims", "Number of observation dimensions"));
    config->push_back(CRP::provided("observation_min", "vector.observation_min", "Lower limit on observations"));
    config->push_back(CRP::provided("observation_max", "vector.observation_max", "Upper limit on observations"));
    config->push_back(CRP::provided("action_dims", "int.action_dims", "Number of action dimensions"));
    config->push_back(CRP::provided("action_min", "vector.action_min", "Lower limit on actions"));
    config->push_back(CRP::provided("action_max", "vector.action_max", "Upper limit on actions"));
    config->push_back(CRP::provided("reward_min", "double.reward_min", "Lower limit on immediate reward"));
    config->push_back(CRP::provided("reward_max", "double.reward_max", "Upper limit on immediate reward"));
  }
  void configure(Configuration &config) override
  {
    timeout = config["timeout"];
    randomization = config["randomization"];
    if (timeout < 0) throw bad_param("task/pendulum/swingup:timeout");
    if (randomization < 0 || randomization > 1) throw bad_param("task/pendulum/swingup:randomization");
    config.set("observation_dims", 2);
    config.set("observation_min", VecD{0., -12 * kPi});
    config.set("observation_max", VecD{2 * kPi, 12 * kPi});
    config.set("action_dims", 1);
    config.set("action_min", VecD{-3});
    config.set("action_max", VecD{3});
    config.set("reward_min", -5 * std::pow(kPi, 2) - 0.1 * std::pow(12 * kPi, 2) - 1 * std::pow(3, 2));
    config.set("reward_max", 0.);
  }
};
GRLX_REGISTER(PendulumSwingupTask)

// dynamics/acrobot, task/acrobot/balancing (acrobot.cpp:36-100): no parameters; the class
// default control step of model/dynamical (0.05 s) applies
struct AcrobotDynamics : Dynamics {
  GRLX_TYPEINFO("dynamics/acrobot")
  int env_id() const override { return GRLX_ENV_ACROBOT; }
};
GRLX_REGISTER(AcrobotDynamics)
struct AcrobotBalancingTask : Task {
  GRLX_TYPEINFO("task/acrobot/balancing")
  int env_id() const override { return GRLX_ENV_ACROBOT; }
  void request(const std::string &, ConfigurationRequest *config) override
  {
    provide_task_outputs(config, "Task limits");
  }
  void configure(Configuration &config) override
  {
    timeout = 20;                                       // acrobot.cpp:125 (fixed)
    config.set("observation_dims", 4);
    config.set("observation_min", VecD{kPi - 12 * kPi / 180, -12 * kPi / 180, -0.6, -1.1});
    config.set("observation_max", VecD{kPi + 12 * kPi / 180, 12 * kPi / 180, 0.6, 1.1});
    config.set("action_dims", 1);
    config.set("action_min", VecD{-1});
    config.set("action_max", VecD{1});
    config.set("reward_min", 1.);
    config.set("reward_max", 1.);
  }
};
GRLX_REGISTER(AcrobotBalancingTask)

// dynamics/cart_pole, task/cart_pole/swingup (cart_pole.cpp:36-56, 110-153)
struct CartPoleDynamics : Dynamics {
  GRLX_TYPEINFO("dynamics/cart_pole")
  int env_id() const override { return GRLX_ENV_CART_POLE; }
  void request(const std::string &, ConfigurationRequest *config) override
  { config->push_back(CRP("end_stop", "Simulate end stops (adds position and velocity to state)", 1)); }
  void configure(Configuration &config) override
  { if ((int)config["end_stop"] != 1) throw Exception(path() + ": end_stop must be 1 (task/cart_pole/swingup needs the 5-dimensional state)"); }
};
GRLX_REGISTER(CartPoleDynamics)
struct CartPoleSwingupTask : Task {
  GRLX_TYPEINFO("task/cart_pole/swingup")
  int end_stop_penalty = 1, action_penalty = 0;
  int env_id() const override { return GRLX_ENV_CART_POLE; }
  void request(const std::string &, ConfigurationRequest *config) override
  {
    config->push_back(CRP("timeout", "Episode timeout", 9.99));
    config->push_back(CRP("randomization", "Start state randomization", 0., CRP::Online));
    config->push_back(CRP("shaping", "Whether to use reward shaping", 0));
    config->push_back(CRP("gamma", "Discount rate for reward shaping", 1.));
    config->push_back(CRP("end_stop_penalty", "Terminate episode with penalty when end stop is reached", 1));
    config->push_back(CRP("action_penalty", "Penalize applied torque", 0));
    provide_task_outputs(config, "Task limits");
  }
  void configure(Configuration &config) override
  {
    timeout = config["timeout"]; randomization = config["randomization"];
    end_stop_penalty = config["end_stop_penalty"]; action_penalty = config["action_penalty"];
    if ((int)config["shaping"] != 0) throw Exception(path() + ": reward shaping is outside the accelerated path");
    config.set("observation_dims", 4);
    config.set("observation_min", VecD{-2.4, 0., -10.0, -5 * kPi});
    config.set("observation_max", VecD{2.4, 2 * kPi, 10.0, 5 * kPi});
    config.set("action_dims", 1);
    config.set("action_min", VecD{-15.});
    config.set("action_max", VecD{15.});
    config.set("reward_min", -2 * std::pow(2.4, 2) - 0.1 * std::pow(10, 2) - std::pow(kPi, 2) - 0.1 * std::pow(5 * kPi, 2) - action_penalty * 2 - end_stop_penalty * 10000);
    config.set("reward_max", 0.);
  }
};
GRLX_REGISTER(CartPoleSwingupTask)


// model/compass_walker (compass_walker.cpp:41-60), task/compass_walker/walk (:198-249)
struct CompassWalkerModel : Model {
  GRLX_TYPEINFO("model/compass_walker")
  double slope_angle = 0.004;
  int env_id() const override { return GRLX_ENV_COMPASS_WALKER; }
  void request(const std::string &, ConfigurationRequest *config) override
  {
    config->push_back(CRP("control_step", "Control step time", 0.2));
    config->push_back(CRP("integration_steps", "Number of integration steps per control step", 20));
    config->push_back(CRP("slope_angle", "Inclination of the slope", 0.004));
  }
  void configure(Configuration &config) override
  {
    control_step = config["control_step"]; integration_steps = config["integration_steps"]; slope_angle = config["slope_angle"];
    if (!(control_step >= 0.001)) throw bad_param("model/compass_walker:control_step");
    if (integration_steps < 1) throw bad_param("model/compass_walker:integration_steps");
  }
};
GRLX_REGISTER(CompassWalkerModel)
struct CompassWalkerWalkTask : Task {
  GRLX_TYPEINFO("task/compass_walker/walk")
  double initial_state_variation = 0.2, slope_angle = 0.004, negative_reward = -100;
  int env_id() const override { return GRLX_ENV_COMPASS_WALKER; }
  void request(const std::string &, ConfigurationRequest *config) override
  {
    config->push_back(CRP("timeout", "Learning episode timeout", 100.));
    config->push_back(CRP("initial_state_variation", "Variation of initial state", 0.2));
    config->push_back(CRP("slope_angle", "Inclination of the slope", 0.004, CRP::System));
    config->push_back(CRP("negative_reward", "Negative reward", -100.));
    config->push_back(CRP("observe", "State elements observed by an agent", VecD{1, 1, 1, 1, 1, 0, 0}));
    config->push_back(CRP("steps", "number of steps after which task is terminated", 0));
    provide_task_outputs(config, "Task limits");
  }
  void configure(Configuration &config) override
  {
    timeout = config["timeout"]; initial_state_variation = config["initial_state_variation"];
    slope_angle = config["slope_angle"]; negative_reward = config["negative_reward"];
    const VecD observe = config["observe"].v();
    if (observe.size() != 7) throw bad_param("task/walk:observe");
    if (observe != VecD{1, 1, 1, 1, 1, 0, 0}) throw Exception(path() + ": only the default observation mask [1,1,1,1,1,0,0] is on the accelerated path");
    if ((int)config["steps"] != 0) throw Exception(path() + ": steps > 0 is outside the accelerated path");
    if (negative_reward > 0) throw bad_param("task/compass_walker/walk:negative_reward");
    config.set("observation_dims", 5);
    config.set("observation_min", VecD{-kPi / 8, -kPi / 4, -kPi, -kPi, 0});
    config.set("observation_max", VecD{kPi / 8, kPi / 4, kPi, kPi, 0.5});
    config.set("action_dims", 1);
    config.set("action_min", VecD{-1.2});
    config.set("action_max", VecD{1.2});
    config.set("reward_min", -101.);
    config.set("reward_max", 50.);
  }
};
GRLX_REGISTER(CompassWalkerWalkTask)

// model/dynamical (modeled.cpp:234-252)
void DynamicalModel::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("control_step", "Control step time", 0.05));
  config->push_back(CRP("integration_steps", "Number of integration steps per control step", 5));
  config->push_back(CRP("dynamics", "dynamics", "Equations of motion", (Configurable *)nullptr));
}
void DynamicalModel::configure(Configuration &config)
{
  dynamics = dynamic_cast<Dynamics *>(config["dynamics"].ptr());
  control_step = config["control_step"];
  integration_steps = config["integration_steps"];
  if (!(control_step >= 0.00001)) throw bad_param("model/dynamical:control_step");
  if (integration_steps < 1) throw bad_param("model/dynamical:integration_steps");
  if (!dynamics) throw Exception(path() + ": dynamics outside the accelerated path");
}
GRLX_REGISTER(DynamicalModel)

// environment/modeled (modeled.cpp:35-119)
void ModeledEnvironment::dims(int *state_dims, int *obs_dims) const { check(grlx_env_dims(task->env_id(), state_dims, obs_dims), path() + ": "); }
void ModeledEnvironment::step(double *state, const double *action, int n, double *obs, double *reward, int32_t *terminal) const
{ // ModeledEnvironment::step for n independent instances, on the GPU
  grlx_config c;
  grlx_config_pendulum_sarsa(&c);
  lower_env(&c);
  int S = 0, D = 0;
  dims(&S, &D);
  c.projector.dims = D + 1;                           // the fine-grained operator only reads the environment fields
  for (int i = 0; i < GRLX_MAX_DIMS; ++i) { c.projector.resolution[i] = 1.; c.projector.wrapping[i] = 0.; }
  check(grlx_env_step(&c, state, action, n, obs, reward, terminal), path() + ": ");
}
void ModeledEnvironment::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("discrete_time", "Always report unit step time", 1));
  config->push_back(CRP("window", "Number of observations to concatenate", 1));
  config->push_back(CRP("stride", "Time steps between concatenated observations", 1));
  config->push_back(CRP("delta", "Action delta for differential actions", VecD{}));
  config->push_back(CRP("model", "model", "Environment model", (Configurable *)nullptr));
  config->push_back(CRP("task", "task", "Task to perform in the environment (should match model)", (Configurable *)nullptr));
  config->push_back(CRP("exporter", "exporter", "Optional exporter for transition log", (Configurable *)nullptr, true));
  provide_task_outputs(config, "Forwarded task parameter");
}
void ModeledEnvironment::configure(Configuration &config)
{
  model = dynamic_cast<Model *>(config["model"].ptr());
  task = dynamic_cast<Task *>(config["task"].ptr());
  discrete_time = config["discrete_time"];
  if (!model || !task) throw Exception(path() + ": model/task outside the accelerated path");
  if ((int)config["window"] != 1 || (int)config["stride"] != 1 || !config["delta"].v().empty())
    throw Exception(path() + ": window/stride/delta are not supported by the accelerated path");
  exporter = config["exporter"].ptr();
  if (discrete_time != 1) throw Exception(path() + ": discrete_time must be 1 on the accelerated path");
  if (model->env_id() != task->env_id()) throw Exception(path() + ": task does not match the model");
  // forward the task's provided parameters (modeled.cpp:79-114)
  Configurator *t = task->configurator;
  for (const char *n : rules::kTaskOutputs) config.set(n, t->child(n)->value);
}
GRLX_REGISTER(ModeledEnvironment)

void ModeledEnvironment::lower_env(grlx_config *c) const
{
  const Model *m = model;
  const Task *t = task;
  c->env = t->env_id();
  c->control_step = m->control_step;
  c->integration_steps = m->integration_steps;
  c->discrete_time = discrete_time;
  c->timeout = t->timeout;
  c->randomization = t->randomization;
  if (const CartPoleSwingupTask *cp = dynamic_cast<const CartPoleSwingupTask *>(t))
  { c->end_stop_penalty = cp->end_stop_penalty; c->action_penalty = cp->action_penalty; }
  if (const CompassWalkerWalkTask *w = dynamic_cast<const CompassWalkerWalkTask *>(t))
  {
    const CompassWalkerModel *wm = dynamic_cast<const CompassWalkerModel *>(m);
    if (!wm || wm->slope_angle != w->slope_angle) throw Exception(w->path() + ": slope_angle must match model/compass_walker");
    c->slope_angle = w->slope_angle; c->initial_state_variation = w->initial_state_variation; c->negative_reward = w->negative_reward;
  }
}

} // namespace grlx_host
