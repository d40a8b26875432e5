/* ref_envs.cpp -- driver around the reference's own acrobot, cart-pole, pendulum and compass-walker sources (TEST INFRASTRUCTURE).
 *
 * oracle/Makefile links this file with the reference's acrobot.cpp, cart_pole.cpp, pendulum.cpp, SWModel.cpp and
 * compass_walker.cpp, compiled unmodified by path against the stand-in header shim/grl/environment.h, into oracle/_ref/ref_envs.
 * The binary is what pins oracle/envs.c's environments (tests/test_oracle_ref_envs.py, bit for bit in libm arithmetic) and what
 * tools/record_ref_envs.py records into tests/golden/ref_envs_*.npz for the GPU test.  This file restates nothing of any
 * environment: every number it prints comes out of a call into the reference's code, with one exception, the *_step commands of
 * the three Dynamics, whose RK4 LOOP is ours (the reference's lives in modeled.cpp, which needs Eigen) around the reference's
 * eom; the two golden files pin that loop in the oracle already.
 *
 * Protocol: one command per stdin line, a word followed by numbers (doubles as C99 hex floats or decimals, read by strtod);
 * one answer per stdout line, doubles as %a, integers as %d / %llu.  "error <text>" answers a line that cannot be served.
 *
 *   acrobot_eom x[5] u                      -> xd[5]                       AcrobotDynamics::eom
 *   acrobot_observe x[5]                    -> obs[4] terminal             AcrobotBalancingTask::observe
 *   acrobot_evaluate x[5] u next[5]         -> reward                      AcrobotBalancingTask::evaluate
 *   acrobot_start d1 d2                     -> x[5]                        AcrobotBalancingTask::start; d1, d2: the two RandGen draws
 *   acrobot_step x[5] u h steps             -> next[5]                     `steps` RK4 sub-steps of h, operation order of modeled.cpp:254-276
 *   cartpole_eom x[5] u                     -> xd[5]                       CartPoleDynamics::eom (end_stop = 1)
 *   cartpole_observe x[5]                   -> obs[4] terminal             CartPoleSwingupTask::observe
 *   cartpole_evaluate x[5] u next[5]        -> reward                      CartPoleSwingupTask::evaluate
 *   cartpole_start d1                       -> x[5]                        CartPoleSwingupTask::start; d1: the RandGen draw
 *   cartpole_step x[5] u h steps            -> next[5]                     the RK4 loop around CartPoleDynamics::eom
 *   cartpole_task timeout randomization end_stop_penalty action_penalty -> ok   CartPoleSwingupTask::configure (shaping 0, gamma 1)
 *   balancing_observe x[5]                  -> obs[4] terminal             CartPoleBalancingTask::observe
 *   balancing_evaluate x[5] u next[5]       -> reward                      CartPoleBalancingTask::evaluate
 *   balancing_start d1                      -> x[5]                        CartPoleBalancingTask::start
 *   balancing_task timeout                  -> ok                          CartPoleBalancingTask::configure
 *   pendulum_eom x[3] u                     -> xd[3]                       PendulumDynamics::eom
 *   pendulum_observe x[3]                   -> obs[2] terminal             PendulumSwingupTask::observe
 *   pendulum_evaluate x[3] u next[3]        -> reward                      PendulumSwingupTask::evaluate
 *   pendulum_start d1 test                  -> x[3]                        PendulumSwingupTask::start
 *   pendulum_actuate u                      -> actuation                   PendulumSwingupTask::actuate (the clamp to +-3)
 *   pendulum_step x[3] u h steps            -> next[3]                     the RK4 loop around PendulumDynamics::eom
 *   pendulum_task timeout randomization     -> ok                          PendulumSwingupTask::configure
 *   walker_step slope tau steps sla ha slar har footx torque -> sla ha slar har footx changed      CSWModel::singleStep
 *   walker_model slope tau steps            -> ok                          CompassWalkerModel::configure
 *   walker_task timeout variation slope negative_reward -> ok              CompassWalkerWalkTask::configure (observe 1 1 1 1 1 0 0, steps 0)
 *   walker_model_step x[11] torque          -> next[11]                    CompassWalkerModel::step
 *   walker_observe x[11]                    -> obs[5] terminal             CompassWalkerWalkTask::observe
 *   walker_evaluate x[11] u next[11]        -> reward                      CompassWalkerWalkTask::evaluate
 *   walker_start seed test                  -> x[11] X                     srand48(seed), CompassWalkerWalkTask::start; X: drand48's 48-bit state after it
 *   walker_start_at X test                  -> x[11] X                     the same from the stream position X (seed48)
 * At start-up the model is configured with slope 0.004, tau 0.2, 20 steps and the task with timeout 100, variation 0.2,
 * slope 0.004, negative reward -100; the cart-pole swing-up task with timeout 9.99, randomization 0 and no penalties, the
 * balancing task with timeout 9.99, the pendulum's with timeout 2.99 and randomization 0.
 * CompassWalkerModel::step never writes next[8] (the step distance): the reference leaves it uninitialised, the stand-in's
 * resize leaves it 0, and the tests do not compare it.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include <grl/environments/acrobot.h>
#include <grl/environments/cart_pole.h>
#include <grl/environments/pendulum.h>
#include <grl/environments/compass_walker/compass_walker.h>

using namespace grl;

static std::deque<double> g_draws;

double ref_envs_rand()
{
  if (g_draws.empty())
    throw Exception("the reference asked for more thread-local draws than the command gave");
  double d = g_draws.front();
  g_draws.pop_front();
  return d;
}

static Vector take(const std::vector<double> &a, size_t at, size_t n)
{
  Vector v;
  for (size_t i = 0; i < n; ++i) v.push(a.at(at + i));
  return v;
}

static void print(const Vector &v)
{
  for (size_t i = 0; i < v.size(); ++i) printf("%s%a", i ? " " : "", v[i]);
}

static Action action_of(double u)
{
  Action a;
  a.v = VectorConstructor(u);
  return a;
}

/* DynamicalModel::step's arithmetic (modeled.cpp:254-276), element by element, around the reference's eom */
static Vector rk4(const Dynamics &dynamics, const Vector &x, const Vector &u, double h, int steps)
{
  Vector next = x, xd, t = x;
  size_t n = x.size();
  std::vector<double> k1(n), k2(n), k3(n), k4(n);
  for (int ii = 0; ii < steps; ++ii)
  {
    dynamics.eom(next, u, &xd);
    for (size_t i = 0; i < n; ++i) { k1[i] = h*xd[i]; t[i] = next[i] + k1[i]/2; }
    dynamics.eom(t, u, &xd);
    for (size_t i = 0; i < n; ++i) { k2[i] = h*xd[i]; t[i] = next[i] + k2[i]/2; }
    dynamics.eom(t, u, &xd);
    for (size_t i = 0; i < n; ++i) { k3[i] = h*xd[i]; t[i] = next[i] + k3[i]; }
    dynamics.eom(t, u, &xd);
    for (size_t i = 0; i < n; ++i) { k4[i] = h*xd[i]; next[i] = next[i] + (k1[i] + 2*k2[i] + 2*k3[i] + k4[i])/6; }
  }
  return next;
}

static unsigned long long rand48_position()
{
  unsigned short zero[3] = {0, 0, 0}, now[3];
  unsigned short *old = seed48(zero);
  memcpy(now, old, sizeof(now));
  seed48(now);
  return (unsigned long long)now[0] | ((unsigned long long)now[1] << 16) | ((unsigned long long)now[2] << 32);
}

static void rand48_seek(unsigned long long x)
{
  unsigned short s[3] = {(unsigned short)(x & 0xffff), (unsigned short)((x >> 16) & 0xffff), (unsigned short)((x >> 32) & 0xffff)};
  seed48(s);
}

struct Driver
{
  AcrobotDynamics acrobot;
  AcrobotBalancingTask balancing;
  CompassWalkerModel walker;
  CompassWalkerWalkTask walk;
  CartPoleDynamics cart_pole;
  CartPoleSwingupTask swingup;
  CartPoleBalancingTask cart_balancing;
  PendulumDynamics pendulum;
  PendulumSwingupTask pendulum_swingup;

  Driver()
  {
    Configuration c;
    c.set("end_stop", 1);
    cart_pole.configure(c);
    pendulum.configure(c);
    configure_swingup(9.99, 0, 0, 0);
    configure_cart_balancing(9.99);
    configure_pendulum(2.99, 0);
    configure_model(0.004, 0.2, 20);
    configure_task(100, 0.2, 0.004, -100);
  }

  void configure_model(double slope, double tau, int steps)
  {
    Configuration c;
    c.set("control_step", tau);
    c.set("integration_steps", steps);
    c.set("slope_angle", slope);
    walker.configure(c);
  }

  void configure_task(double timeout, double variation, double slope, double negative_reward)
  {
    Configuration c;
    c.set("timeout", timeout);
    c.set("initial_state_variation", variation);
    c.set("slope_angle", slope);
    c.set("negative_reward", negative_reward);
    c.set("observe", VectorConstructor(1, 1, 1, 1, 1, 0, 0));
    c.set("steps", 0);
    walk.configure(c);
  }

  void configure_swingup(double timeout, int randomization, int end_stop_penalty, int action_penalty)
  {
    Configuration c;
    c.set("timeout", timeout);
    c.set("randomization", randomization);
    c.set("shaping", 0);
    c.set("gamma", 1.0);
    c.set("end_stop_penalty", end_stop_penalty);
    c.set("action_penalty", action_penalty);
    swingup.configure(c);
  }

  void configure_cart_balancing(double timeout)
  {
    Configuration c;
    c.set("timeout", timeout);
    cart_balancing.configure(c);
  }

  void configure_pendulum(double timeout, double randomization)
  {
    Configuration c;
    c.set("timeout", timeout);
    c.set("randomization", randomization);
    pendulum_swingup.configure(c);
  }

  /* Task::observe / evaluate / start of any task, and Dynamics::eom / the RK4 loop of any dynamics, on S state dimensions */
  void observe(const Task &task, const std::vector<double> &a, size_t S)
  {
    Observation obs; int terminal = -1;
    task.observe(take(a, 0, S), &obs, &terminal);
    print(obs.v); printf(" %d", terminal);
  }

  void evaluate(const Task &task, const std::vector<double> &a, size_t S)
  {
    double reward = 0;
    task.evaluate(take(a, 0, S), action_of(a[S]), take(a, S + 1, S), &reward);
    printf("%a", reward);
  }

  void start(Task &task, const std::vector<double> &draws, int test)
  {
    Vector x;
    g_draws.assign(draws.begin(), draws.end());
    task.start(test, &x);
    if (!g_draws.empty())
      throw Exception("the reference left a thread-local draw unused");
    print(x);
  }

  bool serve_dynamical(const std::string &cmd, const std::vector<double> &a)
  {
    if (cmd == "cartpole_eom" && a.size() == 6)
    {
      Vector xd;
      cart_pole.eom(take(a, 0, 5), take(a, 5, 1), &xd);
      print(xd);
    }
    else if (cmd == "cartpole_observe" && a.size() == 5)
      observe(swingup, a, 5);
    else if (cmd == "cartpole_evaluate" && a.size() == 11)
      evaluate(swingup, a, 5);
    else if (cmd == "cartpole_start" && a.size() == 1)
      start(swingup, a, 0);
    else if (cmd == "cartpole_step" && a.size() == 8)
      print(rk4(cart_pole, take(a, 0, 5), take(a, 5, 1), a[6], (int)a[7]));
    else if (cmd == "cartpole_task" && a.size() == 4)
    {
      configure_swingup(a[0], (int)a[1], (int)a[2], (int)a[3]);
      printf("ok");
    }
    else if (cmd == "balancing_observe" && a.size() == 5)
      observe(cart_balancing, a, 5);
    else if (cmd == "balancing_evaluate" && a.size() == 11)
      evaluate(cart_balancing, a, 5);
    else if (cmd == "balancing_start" && a.size() == 1)
      start(cart_balancing, a, 0);
    else if (cmd == "balancing_task" && a.size() == 1)
    {
      configure_cart_balancing(a[0]);
      printf("ok");
    }
    else if (cmd == "pendulum_eom" && a.size() == 4)
    {
      Vector xd;
      pendulum.eom(take(a, 0, 3), take(a, 3, 1), &xd);
      print(xd);
    }
    else if (cmd == "pendulum_observe" && a.size() == 3)
      observe(pendulum_swingup, a, 3);
    else if (cmd == "pendulum_evaluate" && a.size() == 7)
      evaluate(pendulum_swingup, a, 3);
    else if (cmd == "pendulum_start" && a.size() == 2)
      start(pendulum_swingup, std::vector<double>(1, a[0]), (int)a[1]);
    else if (cmd == "pendulum_actuate" && a.size() == 1)
    {
      Vector actuation;
      pendulum_swingup.actuate(Vector(), Vector(), action_of(a[0]), &actuation);
      print(actuation);
    }
    else if (cmd == "pendulum_step" && a.size() == 6)
      print(rk4(pendulum, take(a, 0, 3), take(a, 3, 1), a[4], (int)a[5]));
    else if (cmd == "pendulum_task" && a.size() == 2)
    {
      configure_pendulum(a[0], a[1]);
      printf("ok");
    }
    else
      return false;
    return true;
  }

  bool serve(const std::string &cmd, const std::vector<double> &a)
  {
    if (serve_dynamical(cmd, a))
      return true;
    if (cmd == "acrobot_eom" && a.size() == 6)
    {
      Vector xd;
      acrobot.eom(take(a, 0, 5), take(a, 5, 1), &xd);
      print(xd);
    }
    else if (cmd == "acrobot_observe" && a.size() == 5)
    {
      Observation obs; int terminal = -1;
      balancing.observe(take(a, 0, 5), &obs, &terminal);
      print(obs.v); printf(" %d", terminal);
    }
    else if (cmd == "acrobot_evaluate" && a.size() == 11)
    {
      double reward = 0;
      balancing.evaluate(take(a, 0, 5), action_of(a[5]), take(a, 6, 5), &reward);
      printf("%a", reward);
    }
    else if (cmd == "acrobot_start" && a.size() == 2)
    {
      Vector x;
      g_draws.assign(a.begin(), a.end());
      balancing.start(0, &x);
      if (!g_draws.empty())
        throw Exception("the reference left a thread-local draw unused");
      print(x);
    }
    else if (cmd == "acrobot_step" && a.size() == 8)
      print(rk4(acrobot, take(a, 0, 5), take(a, 5, 1), a[6], (int)a[7]));
    else if (cmd == "walker_step" && a.size() == 9)
    {
      CSWModel model;
      CSWModelState s;
      model.setSlopeAngle(a[0]);
      model.setTiming(a[1], (int)a[2]);
      s.init(a[7], a[3], a[5], a[4], a[6]);
      model.singleStep(s, a[8]);
      printf("%a %a %a %a %a %d", s.mStanceLegAngle, s.mHipAngle, s.mStanceLegAngleRate, s.mHipAngleRate, s.mStanceFootX, (int)s.mStanceLegChanged);
    }
    else if (cmd == "walker_model" && a.size() == 3)
    {
      configure_model(a[0], a[1], (int)a[2]);
      printf("ok");
    }
    else if (cmd == "walker_task" && a.size() == 4)
    {
      configure_task(a[0], a[1], a[2], a[3]);
      printf("ok");
    }
    else if (cmd == "walker_model_step" && a.size() == 12)
    {
      Vector next;
      walker.step(take(a, 0, 11), take(a, 11, 1), &next);
      print(next);
    }
    else if (cmd == "walker_observe" && a.size() == 11)
    {
      Observation obs; int terminal = -1;
      walk.observe(take(a, 0, 11), &obs, &terminal);
      print(obs.v); printf(" %d", terminal);
    }
    else if (cmd == "walker_evaluate" && a.size() == 23)
    {
      double reward = 0;
      walk.evaluate(take(a, 0, 11), action_of(a[11]), take(a, 12, 11), &reward);
      printf("%a", reward);
    }
    else if ((cmd == "walker_start" || cmd == "walker_start_at") && a.size() == 2)
    {
      Vector x;
      if (cmd == "walker_start")
        srand48((long)a[0]);
      else
        rand48_seek((unsigned long long)a[0]);
      walk.start((int)a[1], &x);
      print(x); printf(" %llu", rand48_position());
    }
    else
      return false;
    return true;
  }
};

int main()
{
  Driver driver;
  char *line = NULL;
  size_t cap = 0;
  while (getline(&line, &cap, stdin) > 0)
  {
    std::vector<double> args;
    char *save = NULL, *word = strtok_r(line, " \t\r\n", &save);
    if (!word)
      continue;
    std::string cmd = word;
    bool parsed = true;
    while ((word = strtok_r(NULL, " \t\r\n", &save)))
    {
      char *end = NULL;
      args.push_back(strtod(word, &end));
      parsed = parsed && end != word && *end == 0;
    }
    try
    {
      if (!parsed || !driver.serve(cmd, args))
        printf("error unknown command or wrong argument count: %s", cmd.c_str());
    }
    catch (const Exception &e)
    {
      printf("error %s", e.what().c_str());
    }
    catch (const std::exception &e)
    {
      printf("error %s", e.what());
    }
    printf("\n");
    fflush(stdout);
  }
  free(line);
  return 0;
}
