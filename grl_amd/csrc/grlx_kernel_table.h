// grlx_kernel_table.h -- every rollout instantiation of the library, one row each (KernelRow, grlx_internal.h).
//
// Included at the end of grlx_kernels.hip: taking a kernel's address here is what instantiates it.  To add an instantiation, add its row
// and its case in tests/kernel_plan_cases.py (a launched case is held to the oracle's bits by tests/test_gpu_kernel_plan_parity.py);
// plan_rollout (grlx_plan.cpp) takes the FIRST row whose key -- family, environment, actions, replicas per wave, mode, and for FAM_TGT the
// (target, safe) pair -- and whose `matches` fit the launch, so the rows stand in precedence order:
//   sweep -> wide served -> served -> stamped deferred -> tapped deferred -> advantage -> 32 -> 16 -> 8 -> specialised 4 -> generic 4
// and a specialised row stands before the generic row of the same key.  Admission at create asks the same rows (kernel_built).
#pragma once

namespace grlx {

// the instantiation, once: its spelling and its address
#define GRLX_K(...) #__VA_ARGS__, reinterpret_cast<const void *>(&__VA_ARGS__)
#define GRLX_UNSERVED "", nullptr, 0
#define P_ GRLX_ENV_PENDULUM
#define A_ GRLX_ENV_ACROBOT
#define C_ GRLX_ENV_CART_POLE
#define W_ GRLX_ENV_COMPASS_WALKER
#define GEN nullptr, GRLX_KERNEL_GENERIC
#define INP nullptr, GRLX_KERNEL_IN_PLACE
#define SPEC(S) &S::matches, GRLX_KERNEL_SPECIALISED
template <int AGENT> using TcA = SpecPendulumTcA<AGENT>;

const KernelRow *kernel_rows(int *count)
{
  static const KernelRow rows[] = {
    // family env A layout mode       target safe  matches / variant             rollout kernel                                                    server, mailbox
    // ---- SARSA / Q / Expected SARSA / advantage learning, replacing trace or none
    {FAM_TD, P_, 3, 8, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_wide_sweep_kernel<GRLX_ENV_PENDULUM, 3>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 4, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_sweep_kernel<GRLX_ENV_PENDULUM, 3>), GRLX_UNSERVED},
    {FAM_TD, P_, 5, 8, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_wide_sweep_kernel<GRLX_ENV_PENDULUM, 5>), GRLX_UNSERVED},
    {FAM_TD, P_, 5, 4, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_sweep_kernel<GRLX_ENV_PENDULUM, 5>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 8, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_wide_sweep_kernel<GRLX_ENV_ACROBOT, 3>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 4, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_sweep_kernel<GRLX_ENV_ACROBOT, 3>), GRLX_UNSERVED},
    {FAM_TD, C_, 3, 8, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_wide_sweep_kernel<GRLX_ENV_CART_POLE, 3>), GRLX_UNSERVED},
    {FAM_TD, C_, 3, 4, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_sweep_kernel<GRLX_ENV_CART_POLE, 3>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 8, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_wide_sweep_kernel<GRLX_ENV_COMPASS_WALKER, 3>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 4, MODE_SWEEP,     0, 0, GEN, GRLX_K(rollout_sweep_kernel<GRLX_ENV_COMPASS_WALKER, 3>), GRLX_UNSERVED},
    // the server gets the numeric parameters of its rollout kernel (same constants, same folding): they stand in one row
    {FAM_TD, W_, 3, 8, MODE_SERVED,    0, 0, SPEC(SpecWalkerQ), GRLX_K(rollout_wide_served_kernel<GRLX_ENV_COMPASS_WALKER, SpecWalkerQ>), GRLX_K(env_server_walker_kernel<SpecWalkerQ>), kWideMailBytes},
    {FAM_TD, A_, 3, 8, MODE_SERVED,    0, 0, SPEC(SpecAcrobotQ), GRLX_K(rollout_wide_served_kernel<GRLX_ENV_ACROBOT, SpecAcrobotQ>), GRLX_K(env_server_acrobot_pinned_kernel<SpecAcrobotQ>), kWideMailBytes},
    {FAM_TD, A_, 3, 8, MODE_SERVED,    0, 0, GEN, GRLX_K(rollout_wide_served_kernel<GRLX_ENV_ACROBOT, SpecNone>), GRLX_K(env_server_acrobot_kernel<SpecNone>), kWideMailBytes},
    {FAM_TD, W_, 3, 8, MODE_SERVED,    0, 0, GEN, GRLX_K(rollout_wide_served_kernel<GRLX_ENV_COMPASS_WALKER, SpecNone>), GRLX_K(env_server_walker_kernel<SpecNone>), kWideMailBytes},
    {FAM_TD, P_, 3, 4, MODE_SERVED,    0, 0, SPEC(TcA<GRLX_AGENT_SARSA>), GRLX_K(rollout_served_kernel<3, SpecPendulumTcA<GRLX_AGENT_SARSA>>), GRLX_K(env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumTcA<GRLX_AGENT_SARSA>>), kEnvMailBytes},
    {FAM_TD, P_, 3, 4, MODE_SERVED,    0, 0, SPEC(TcA<GRLX_AGENT_Q>), GRLX_K(rollout_served_kernel<3, SpecPendulumTcA<GRLX_AGENT_Q>>), GRLX_K(env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumTcA<GRLX_AGENT_Q>>), kEnvMailBytes},
    {FAM_TD, P_, 3, 4, MODE_SERVED,    0, 0, SPEC(TcA<GRLX_AGENT_EXPECTED_SARSA>), GRLX_K(rollout_served_kernel<3, SpecPendulumTcA<GRLX_AGENT_EXPECTED_SARSA>>), GRLX_K(env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumTcA<GRLX_AGENT_EXPECTED_SARSA>>), kEnvMailBytes},
    {FAM_TD, P_, 3, 4, MODE_SERVED,    0, 0, GEN, GRLX_K(rollout_served_kernel<3, SpecNone>), GRLX_K(env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecNone>), kEnvMailBytes},
    {FAM_TD, P_, 3, 4, MODE_STAMPED,   0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone, true>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 4, MODE_TAPPED,    0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecNone, true, false, true>), GRLX_UNSERVED},
    {FAM_TD, P_, 5, 4, MODE_TAPPED,    0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 5, false, SpecNone, true, false, true>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 4, MODE_TAPPED,    0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_ACROBOT, 3, false, SpecNone, true, false, true>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 4, MODE_ADVANTAGE, 0, 0, INP, GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone, false, true>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 4, MODE_ADVANTAGE, 0, 0, INP, GRLX_K(rollout_kernel<GRLX_ENV_ACROBOT, 3, true, SpecNone, false, true>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 32, MODE_DEFERRED, 0, 0, SPEC(SpecWalkerQ), GRLX_K(rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 8, SpecWalkerQ>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 32, MODE_DEFERRED, 0, 0, GEN, GRLX_K(rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 8, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 16, MODE_DEFERRED, 0, 0, SPEC(SpecWalkerQ), GRLX_K(rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 4, SpecWalkerQ>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 16, MODE_DEFERRED, 0, 0, SPEC(SpecAcrobotQ), GRLX_K(rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 4, SpecAcrobotQ>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 16, MODE_DEFERRED, 0, 0, GEN, GRLX_K(rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 4, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 16, MODE_DEFERRED, 0, 0, GEN, GRLX_K(rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 4, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 8, MODE_DEFERRED,  0, 0, SPEC(TcA<GRLX_AGENT_SARSA>), GRLX_K(rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecPendulumTcA<GRLX_AGENT_SARSA>>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 8, MODE_DEFERRED,  0, 0, SPEC(TcA<GRLX_AGENT_Q>), GRLX_K(rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecPendulumTcA<GRLX_AGENT_Q>>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 8, MODE_DEFERRED,  0, 0, SPEC(SpecWalkerQ), GRLX_K(rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 2, SpecWalkerQ>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 8, MODE_DEFERRED,  0, 0, SPEC(SpecAcrobotQ), GRLX_K(rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 2, SpecAcrobotQ>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 8, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, P_, 5, 8, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_wide_kernel<GRLX_ENV_PENDULUM, 5, 2, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 8, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 2, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, C_, 3, 8, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_wide_kernel<GRLX_ENV_CART_POLE, 3, 2, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 8, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 2, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 4, MODE_DEFERRED,  0, 0, SPEC(TcA<GRLX_AGENT_SARSA>), GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecPendulumTcA<GRLX_AGENT_SARSA>>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 4, MODE_DEFERRED,  0, 0, SPEC(TcA<GRLX_AGENT_Q>), GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecPendulumTcA<GRLX_AGENT_Q>>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 4, MODE_DEFERRED,  0, 0, SPEC(TcA<GRLX_AGENT_EXPECTED_SARSA>), GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecPendulumTcA<GRLX_AGENT_EXPECTED_SARSA>>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 4, MODE_DEFERRED,  0, 0, SPEC(SpecWalkerQ), GRLX_K(rollout_kernel<GRLX_ENV_COMPASS_WALKER, 3, false, SpecWalkerQ>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 4, MODE_DEFERRED,  0, 0, SPEC(SpecAcrobotQ), GRLX_K(rollout_kernel<GRLX_ENV_ACROBOT, 3, false, SpecAcrobotQ>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 4, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, P_, 3, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, P_, 5, 4, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 5, false, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, P_, 5, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_kernel<GRLX_ENV_PENDULUM, 5, true, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 4, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_ACROBOT, 3, false, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, A_, 3, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_kernel<GRLX_ENV_ACROBOT, 3, true, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, C_, 3, 4, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_CART_POLE, 3, false, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, C_, 3, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_kernel<GRLX_ENV_CART_POLE, 3, true, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 4, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_kernel<GRLX_ENV_COMPASS_WALKER, 3, false, SpecNone>), GRLX_UNSERVED},
    {FAM_TD, W_, 3, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_kernel<GRLX_ENV_COMPASS_WALKER, 3, true, SpecNone>), GRLX_UNSERVED},
    // ---- actor-critic (no discretised actions: A = 0).  In place: taps, or a context without a trace; 16 / 12 / 8: B = 4 / 3 / 2 sub-batches
    {FAM_AC, C_, 0, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecNone, false>), GRLX_UNSERVED},
    {FAM_AC, P_, 0, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_ac_kernel<GRLX_ENV_PENDULUM, SpecNone, false>), GRLX_UNSERVED},
    {FAM_AC, C_, 0, 16, MODE_DEFERRED, 0, 0, SPEC(SpecCartPoleAc), GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 4, SpecCartPoleAc>), GRLX_UNSERVED},
    {FAM_AC, C_, 0, 16, MODE_DEFERRED, 0, 0, GEN, GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 4, SpecNone>), GRLX_UNSERVED},
    {FAM_AC, P_, 0, 16, MODE_DEFERRED, 0, 0, GEN, GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_PENDULUM, 4, SpecNone>), GRLX_UNSERVED},
    {FAM_AC, C_, 0, 12, MODE_DEFERRED, 0, 0, SPEC(SpecCartPoleAc), GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 3, SpecCartPoleAc>), GRLX_UNSERVED},
    {FAM_AC, C_, 0, 12, MODE_DEFERRED, 0, 0, GEN, GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 3, SpecNone>), GRLX_UNSERVED},
    {FAM_AC, P_, 0, 12, MODE_DEFERRED, 0, 0, GEN, GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_PENDULUM, 3, SpecNone>), GRLX_UNSERVED},
    {FAM_AC, C_, 0, 8, MODE_DEFERRED,  0, 0, SPEC(SpecCartPoleAc), GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 2, SpecCartPoleAc>), GRLX_UNSERVED},
    {FAM_AC, C_, 0, 8, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 2, SpecNone>), GRLX_UNSERVED},
    {FAM_AC, P_, 0, 8, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_ac_wide_kernel<GRLX_ENV_PENDULUM, 2, SpecNone>), GRLX_UNSERVED},
    {FAM_AC, C_, 0, 4, MODE_DEFERRED,  0, 0, SPEC(SpecCartPoleAc), GRLX_K(rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecCartPoleAc, true>), GRLX_UNSERVED},
    {FAM_AC, C_, 0, 4, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecNone, true>), GRLX_UNSERVED},
    {FAM_AC, P_, 0, 4, MODE_DEFERRED,  0, 0, GEN, GRLX_K(rollout_ac_kernel<GRLX_ENV_PENDULUM, SpecNone, true>), GRLX_UNSERVED},
    // ---- predictor/critic/qv
    {FAM_QV, P_, 3, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_qv_kernel<GRLX_ENV_PENDULUM, 3>), GRLX_UNSERVED},
    {FAM_QV, A_, 3, 4, MODE_IN_PLACE,  0, 0, INP, GRLX_K(rollout_qv_kernel<GRLX_ENV_ACROBOT, 3>), GRLX_UNSERVED},
    // ---- accumulating trace: one ordering; the DEFERRED rows are the ones that record no taps
    {FAM_ACC, P_, 3, 4, MODE_DEFERRED, 0, 0, SPEC(SpecPendulumAcc<GRLX_AGENT_SARSA>), GRLX_K(rollout_acc_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumAcc<GRLX_AGENT_SARSA>>), GRLX_UNSERVED},
    {FAM_ACC, P_, 3, 4, MODE_DEFERRED, 0, 0, SPEC(SpecPendulumAcc<GRLX_AGENT_Q>), GRLX_K(rollout_acc_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumAcc<GRLX_AGENT_Q>>), GRLX_UNSERVED},
    {FAM_ACC, P_, 3, 4, MODE_IN_PLACE, 0, 0, INP, GRLX_K(rollout_acc_kernel<GRLX_ENV_PENDULUM, 3>), GRLX_UNSERVED},
    {FAM_ACC, A_, 3, 4, MODE_IN_PLACE, 0, 0, INP, GRLX_K(rollout_acc_kernel<GRLX_ENV_ACROBOT, 3>), GRLX_UNSERVED},
    // ---- target network and / or claim table (projector/tile_coding:safe) of the Q table
    {FAM_TGT, P_, 3, 4, MODE_IN_PLACE, 1, 0, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_PENDULUM, 3, true, false>), GRLX_UNSERVED},
    {FAM_TGT, P_, 3, 4, MODE_IN_PLACE, 0, 1, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_PENDULUM, 3, false, true>), GRLX_UNSERVED},
    {FAM_TGT, P_, 3, 4, MODE_IN_PLACE, 1, 1, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_PENDULUM, 3, true, true>), GRLX_UNSERVED},
    {FAM_TGT, A_, 3, 4, MODE_IN_PLACE, 1, 0, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_ACROBOT, 3, true, false>), GRLX_UNSERVED},
    {FAM_TGT, A_, 3, 4, MODE_IN_PLACE, 0, 1, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_ACROBOT, 3, false, true>), GRLX_UNSERVED},
    {FAM_TGT, C_, 3, 4, MODE_IN_PLACE, 1, 0, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_CART_POLE, 3, true, false>), GRLX_UNSERVED},
    {FAM_TGT, C_, 3, 4, MODE_IN_PLACE, 0, 1, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_CART_POLE, 3, false, true>), GRLX_UNSERVED},
    {FAM_TGT, W_, 3, 4, MODE_IN_PLACE, 1, 0, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_COMPASS_WALKER, 3, true, false>), GRLX_UNSERVED},
    {FAM_TGT, W_, 3, 4, MODE_IN_PLACE, 0, 1, INP, GRLX_K(rollout_tgt_kernel<GRLX_ENV_COMPASS_WALKER, 3, false, true>), GRLX_UNSERVED},
  };
  *count = (int)(sizeof(rows) / sizeof(rows[0]));
  return rows;
}

#undef GRLX_K
#undef GRLX_UNSERVED
#undef P_
#undef A_
#undef C_
#undef W_
#undef GEN
#undef INP
#undef SPEC

} // namespace grlx
