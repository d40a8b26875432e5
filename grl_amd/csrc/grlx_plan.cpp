// grlx_plan.cpp -- which kernel a launch runs, decided in one place.
//
// plan_rollout reads the rows of grlx_kernel_table.h and returns the row, the grid and the server of ONE launch; choose_layout gives a
// context its replicas per wave; kernel_built answers the admission checks of grlx_create from the same rows.  All three are pure
// functions: no device, no allocation, no environment variable.  launch_plan executes a plan.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "grlx_internal.h"

namespace grlx {

bool kernel_built(int family, int env, int actions, int replicas_per_wave, int mode, int target, int safe)
{
  int n;
  const KernelRow *rows = kernel_rows(&n);
  for (int i = 0; i < n; ++i)
  {
    const KernelRow &r = rows[i];
    if (r.family == family && r.env == env && r.actions == actions && r.replicas_per_wave == replicas_per_wave && r.mode == mode &&
        r.target == target && r.safe == safe)
      return true;
  }
  return false;
}

// replicas per wave: wide waves once the batch outnumbers the SIMDs four to one (taps: always 4)
Layout choose_layout(const grlx_config &cfg, int simds)
{
  const int N = cfg.n_replicas, per_simd = (N + simds - 1) / simds;
  const bool td = is_td_agent(cfg.agent), ac = cfg.agent == GRLX_AGENT_AC, automatic = cfg.replicas_per_wave == 0;
  const bool has_wide = cfg.target_interval == 0 && cfg.projector.safe == 0 && (td || ac) && cfg.trace != GRLX_TRACE_ACCUMULATING;
  Layout L;
  // 8 once the 4-replica waves outnumber the SIMDs.  (Round 2's 16-slot actor-critic kernel parked four sub-batches in 66 KB of LDS,
  // two waves per CU: 213 M vs 329 M env-steps/s at 16384 cart-pole replicas.  Since round 3 the sub-batches beyond the second park in
  // device memory)
  int rpw = automatic ? (((N + kReplicasPerWave - 1) / kReplicasPerWave > simds) ? 8 : 4) : cfg.replicas_per_wave;
  // actor-critic, more than 8 replicas per SIMD: more slots per wave share one environment phase (grlx_rollout_ac_wide.h; 16384 cart-pole
  // replicas: 373 M env-steps/s with 8 slots, 405 M with 12, 425 M with 16).  16 slots for 15 or more replicas per SIMD; 12, rotated
  // trial by trial over the wave's own replicas, for 9 to 14 (13 replicas keep 12 slots busier than 16).
  if (automatic && ac && rpw == 8 && cfg.wave_limit == 0)
    rpw = per_simd >= 15 ? 16 : per_simd >= 9 ? 12 : 8;
  // TD agents, 15 (30) or more replicas per SIMD: four (eight) sub-batches per wave share one environment phase, where that is built --
  // where the environment phase is half of a pass (the acrobot and the compass walker; 32: the walker, two lanes per replica suffice)
  if (automatic && !ac && rpw == 8)
  {
    if (per_simd >= 30 && kernel_built(FAM_TD, cfg.env, cfg.action_steps, 32, MODE_DEFERRED)) rpw = 32;
    else if (per_simd >= 15 && kernel_built(FAM_TD, cfg.env, cfg.action_steps, 16, MODE_DEFERRED)) rpw = 16;
  }
  if (!has_wide || (cfg.tap_replica >= 0 && cfg.tap_capacity > 0)) rpw = 4;
  // without a trace (see grlx_ctx): what runs is the sweep kernels' layouts (4, 8) or the in-place actor-critic kernel (4)
  L.no_trace_td = cfg.trace == GRLX_TRACE_NONE && td && cfg.target_interval == 0 && cfg.projector.safe == 0 && cfg.env != GRLX_ENV_EXTERNAL;
  L.no_trace_ac = cfg.trace == GRLX_TRACE_NONE && ac && cfg.env != GRLX_ENV_EXTERNAL;
  if (L.no_trace_td && rpw > 8) rpw = 8;
  if (L.no_trace_ac) rpw = 4;
  L.replicas_per_wave = rpw;
  L.wave_limit = cfg.wave_limit > 0 ? cfg.wave_limit : simds;      // these kernels hold a SIMD's whole register file: one wave per SIMD
  return L;
}

KernelPlan plan_rollout(const DevParams &P, const PlanFacts &facts)
{
  const int family = P.agent == GRLX_AGENT_AC ? FAM_AC : P.agent == GRLX_AGENT_QV ? FAM_QV : (P.target_interval > 0 || P.tile_safe != 0) ? FAM_TGT :
                     P.trace_kind == GRLX_TRACE_ACCUMULATING ? FAM_ACC : FAM_TD;
  const bool td = is_td_agent(P.agent), adv = P.agent == GRLX_AGENT_ADVANTAGE;
  // stamps and per-step taps are recorded by the instantiation that updates in place
#ifdef GRLX_WIDE_STAMPS
  const bool in_place = tapped(P);                   // stamped wide build: diag_out feeds the wide kernel
#else
  const bool in_place = records(P);
#endif
  // which modes this launch may run; the rows' order decides among them
  bool on[MODE_IN_PLACE + 1] = {};
  int R = P.replicas_per_wave;
  KernelPlan plan = {};
  switch (family)
  {
    case FAM_TD:
      // a sweep runs the SpecSweep rows or nothing: never the shared values
      if (facts.sweep) { on[MODE_SWEEP] = !records(P) && td && !P.env_mail; break; }
      on[MODE_SERVED] = facts.server && !records(P) && td;
      on[MODE_STAMPED] = P.diag_out && P.diag_deferred && !tapped(P);
      on[MODE_TAPPED] = P.tap_deferred && tapped(P) && !P.diag_out && !adv;
      on[MODE_ADVANTAGE] = adv;
      on[MODE_IN_PLACE] = in_place && !adv && !on[MODE_TAPPED];
      on[MODE_DEFERRED] = !in_place && !adv;
      break;
    case FAM_AC:
      // taps are recorded by the in-place instantiation; a context without a trace runs it too: the deferred critic update stores p's
      // weight behind the loads of V(s') already in flight, and without a trace nothing forwards it to them
      on[MODE_IN_PLACE] = facts.ac_in_place || tapped(P);
      on[MODE_DEFERRED] = !on[MODE_IN_PLACE];
      break;
    case FAM_ACC:
      on[MODE_DEFERRED] = !tapped(P);
      on[MODE_IN_PLACE] = true;
      break;
    default:
      on[MODE_IN_PLACE] = true;
  }
  if (family == FAM_AC && on[MODE_DEFERRED] && R >= 8)
  { // two (three, four) sub-batches per wave share one environment phase (grlx_rollout_ac_wide.h); at most wave_limit waves, the
    // replicas beyond their first load are handed out by a device-side counter as slots fall idle
    auto limited = [&](int r) { const int all = (P.n_replicas + r - 1) / r; return all < P.wave_limit ? all : P.wave_limit; };
    int waves = limited(R);
    // 12 slots: every wave owns ceil(n / waves) consecutive replicas and rotates them through its slots (no device-wide queue); a batch
    // that would give a wave more than kAcOwnedMax runs in the 8-slot kernel (grlx_replicas_per_wave goes on reporting 12)
    if (R == 12 && (P.n_replicas + waves - 1) / waves > kAcOwnedMax) waves = limited(R = 8);
    if (R == 12)
    { // (with K = ceil(n / waves) replicas per wave the last waves may own none: launch only the ones that own some)
      const int k = (P.n_replicas + waves - 1) / waves;
      waves = (P.n_replicas + k - 1) / k;
    }
    plan.grid = (unsigned)waves;
    plan.set_queue = true;
    plan.queue_word = (uint32_t)waves * (uint32_t)R;
  }
  int n;
  const KernelRow *rows = kernel_rows(&n);
  for (int i = 0; i < n; ++i)
  {
    const KernelRow &r = rows[i];
    // only the rows that record nothing come in several layouts; the others run four replicas per wave whatever the context's layout
    const bool layout_keyed = r.mode == MODE_SWEEP || r.mode == MODE_SERVED || r.mode == MODE_DEFERRED;
    if (r.family != family || !on[r.mode] || r.env != P.env || r.actions != P.A || (layout_keyed && r.replicas_per_wave != R)) continue;
    if (family == FAM_TGT && (r.target != (P.target_interval > 0) || r.safe != (P.tile_safe != 0))) continue;
    if (r.matches && (P.no_specialisation || !r.matches(P))) continue;
    if (r.mode == MODE_SERVED && r.replicas_per_wave == 8)
    { // The walker's server is built and tested but NOT the default: beside the 346-register rollout wave it has 160 registers, too few to
      // hold the sine's constants and the integrator's stages, and the code it becomes issues more vector instructions than the SIMD has
      // slots left (measured: 180-213 M env-steps/s with it against 220 M without).
      // A server that cannot be resident beside its rollout wave would only be waited for in vain (8000 polls at the first step).
      // Either way the launch goes unserved: the generic pair is not tried in place of the specialised one.
      if ((P.env == GRLX_ENV_COMPASS_WALKER && !facts.walker_server) || !facts.fits(r)) { on[MODE_SERVED] = false; continue; }
    }
    plan.row = &r;
    plan.server = r.mode == MODE_SERVED;
    if (!plan.set_queue) plan.grid = (unsigned)((P.n_replicas + r.replicas_per_wave - 1) / r.replicas_per_wave);
    return plan;
  }
  return KernelPlan{};
}

// do a wave of the rollout kernel and a wave of its server fit on one SIMD together (512 registers)?  asked of the runtime once per row
bool waves_fit_together(const KernelRow &row)
{
  int n;
  const KernelRow *rows = kernel_rows(&n);
  static std::vector<signed char> known((size_t)n, -1);
  signed char &fit = known[(size_t)(&row - rows)];
  if (fit >= 0) return fit != 0;
  fit = 0;
  hipFuncAttributes a, b;
  if (hipFuncGetAttributes(&a, row.kernel) != hipSuccess || hipFuncGetAttributes(&b, row.server) != hipSuccess)
  {
    (void)hipGetLastError();
    return false;
  }
  const int gran = 8;                                  // allocation granule of the unified register file
  const int ra = (a.numRegs + gran - 1) / gran * gran, rb = (b.numRegs + gran - 1) / gran * gran;
  if (getenv("GRLX_ENV_SERVER_DEBUG"))
    fprintf(stderr, "grlx: rollout wave %d registers (%zu B scratch, %zu B LDS) + server wave %d registers (%zu B scratch): %s\n", a.numRegs, a.localSizeBytes,
            a.sharedSizeBytes, b.numRegs, b.localSizeBytes, ra + rb <= 512 ? "resident together" : "do not fit one SIMD");
  fit = ra + rb <= 512;
  return fit != 0;
}

hipError_t launch_plan(const KernelPlan &plan, const DevParams &P, int n_trials, const SweepParams *sweep, hipStream_t stream, hipStream_t server)
{
  if (!plan.row) return hipErrorInvalidValue;
  const KernelRow &r = *plan.row;
  if (r.replicas_per_wave == 32 && !P.park) return hipErrorInvalidValue;      // the sub-batches beyond the third park there
  if (r.mode == MODE_SWEEP && !sweep) return hipErrorInvalidValue;
  if (plan.server && !P.env_mail) return hipErrorInvalidValue;
  hipError_t e;
  void *args[3] = {const_cast<DevParams *>(&P), &n_trials, &sweep};
  if (plan.set_queue && (e = launch_set_u32(P.queue, plan.queue_word, stream)) != hipSuccess) return e;
  // one server block per rollout wave
  if (plan.server && (e = hipLaunchKernel(r.server, dim3(plan.grid), dim3(64), args, 0, server)) != hipSuccess) return e;
  return hipLaunchKernel(r.kernel, dim3(plan.grid), dim3(64), args, 0, stream);
}

} // namespace grlx
