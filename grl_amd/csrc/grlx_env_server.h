// grlx_env_server.h -- the environment step of the 4-replicas-per-wave pendulum kernels, moved to a SECOND kernel that shares the SIMDs.
// Part of the single translation unit grlx_kernels.hip (included there, in order; not self-contained).
//
// Why.  At 4096 replicas the rollout kernel runs exactly one wave per SIMD and issues on 0.64 of its cycles; the rest is latency of its
// own dependent instructions (f64 chains of the sine, LDS round trips), which only another wave on the SIMD could fill -- and a second
// 384-register wave does not fit.  But the RK4 integration (40 % of a pass) needs few registers, reads no table, and its inputs are known
// early: the next step is taken from the state this pass started in, with one of NA known torques.  So a small kernel -- one 64-thread
// block per rollout wave, 96 registers beside the 416 of rollout_served_kernel, resident on the same SIMDs (tools/microbench/coresident.hip:
// both kernels stay resident, a round trip between them through device memory costs 3.8 k cycles) -- integrates the steps AHEAD of the
// rollout wave, for every action it can choose (two levels: see env_server_kernel), while the rollout wave works through its table
// phase; the rollout wave then only fetches the result of the action its sampler chose.  Same operations on the same arguments (env_step
// is the same code): same bits.  DESIGN.md section 4.1g has the measurements.
//
// Protocol, one 1-KB mailbox per replica (EnvMail).  Every payload word travels in a 16-byte UNIT {value, seq} written by one lane with one
// 16-byte store and read with one 16-byte load (device scope, sc1: served by memory that every XCD sees): a unit is either the old or the
// new one, and says which -- no ordering between accesses is needed, a reader that finds a wrong seq reads again.
//   rollout wave -> server: cmd[seq & 3] = seq << 8 | op, seq = 1, 2, ...;  op 0..NA-1: "the step was taken with action op",
//                           op kReset: "a trial starts in reset[]" (units tagged seq), op kExit: "no further command".
//   server -> rollout wave: cand[seq & 1][a] = units {x0, x1, x2, obs0, reward} after command seq, stepped with action a (obs1 = x1;
//                           terminal and the domain check are comparisons on x the rollout wave redoes).  Two buffers: the server writes
//                           the candidates of command seq + 1 while the rollout wave may still be reading those of command seq.
//                           In memory a buffer of the specialised pairs (SPEC::kCandByUnit) is laid out unit by unit, [seq & 1][unit][a]:
//                           each of the server's five store instructions then writes its three units side by side, 48 contiguous bytes
//                           of one 64-byte block.  Measured: the headline launch is a few per cent shorter that way.  The supposed reason,
//                           which no counter has confirmed, is that the three become one write to memory.
// The rollout wave never depends on the server: a fetch that does not arrive within kFetchPolls polls is computed locally (it has the state
// and the action), the replica tells the server to stop and integrates by itself for the rest of the launch.  The server leaves when every
// replica of its block has sent kExit (or has gone on without it), or after kServerStartPolls polls without a first command /
// kServerIdlePolls polls (or iterations that consume no command) without a further one.  Neither side can hang the other.
// The pass of the rollout wave exists twice (rollout_body, grlx_rollout.h): a full wave whose four replicas are all served and in mid-episode
// takes its answers with ONE vote of the whole wave (mail_take_wave) in a loop of straight-line passes; a take that runs into its bound
// there changes nothing and leaves that loop, and the general pass takes the same step again with mail_take, per replica, as described above.
// The early take (SPEC::kEarlyTake, the specialised instantiations).  cand[n & 1][.] is stored the moment command n arrives -- a pass before
// the sampler that chooses among its three states.  Inside that loop a pass therefore loads all fifteen units of cand[n & 1] during its
// table phase (mail_prefetch_all), votes on their tags once its sampler has chosen (mail_vote_all, the same bound) and hands the chosen
// candidate round (mail_hand_round): no trip through memory between the choice and the next state, and mail_take_wave is left with the
// first pass of every visit to the loop.  A vote that runs into its bound changes nothing: the pass sends its command, issues the classic
// mail_prefetch and leaves the loop, as above.  Such a pass loads 256 B per replica from the mailbox where the others load 80 B.
#pragma once

namespace grlx {

struct __attribute__((aligned(16))) MailUnit { double v; unsigned long long seq; };
constexpr int kCandUnits = 5;
constexpr int kCandSlots = 4;                 // EnvMail::cand: four unit slots (64 B) per unit index, one per action, three of them used
struct __attribute__((aligned(1024))) EnvMail {
  unsigned long long cmd[4];                    //   0
  MailUnit reset[3];                            //  32
  unsigned long long pad0[6];                   //  80
  unsigned long long stats[16];                 // 128  ([15]: served to the end 1 / fell back 2; [14]: passes of the replica's wave in the
                                                //       wave-uniform loop; the rest: GRLX_ENV_SERVER_STATS builds)
  union {                                       // 256 .. 896: ONE of the two layouts per launch, that of the kernel pair (SPEC::kCandByUnit)
    MailUnit by_unit[2][kCandUnits][kCandSlots];  //   [seq & 1][unit][action slot]: unit by unit, the actions side by side
    MailUnit by_cand[2][3][kCandUnits];           //   [seq & 1][action][unit], the first 480 B (the generic pair)
  } cand;
  unsigned long long pad1[16];                  // 896  ([0..7]: the rollout wave's stamps, GRLX_ENV_SERVER_STATS builds)
};
static_assert(sizeof(EnvMail) == kEnvMailBytes, "one mailbox = kEnvMailBytes");
static_assert(offsetof(EnvMail, stats) + 15 * sizeof(unsigned long long) == kEnvMailFlagOffset, "the flag grlx_env_server_counts reads");
static_assert(offsetof(EnvMail, stats) + 14 * sizeof(unsigned long long) == kEnvMailUniformOffset, "the count grlx_uniform_pass_counts reads");

typedef __attribute__((address_space(1))) unsigned long long env_gu64;
typedef unsigned int mail_u32x4 __attribute__((ext_vector_type(4)));
#define GRLX_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
constexpr unsigned kMailReset = 3u, kMailExit = 4u;
constexpr unsigned kFetchPolls = 400u;              // x (one round trip through memory) = ~0.4 ms: the server is not there.  (A take that
                                                    //   gives up inside the wave-uniform pass, mail_take_wave, is repeated by the general pass:
                                                    //   for that ONE pass the bound on a missing server doubles, to about 0.8 ms)
constexpr unsigned kFirstFetchPolls = 8000u;        // the first answer of a launch: the two kernels start on two streams, and the first
                                                    //   launch of a kernel in a process may wait for its scratch to be set up
constexpr unsigned kServerStartPolls = 20000u;      // x (s_sleep + one round trip) = tens of ms without a first command: the rollout kernel is
                                                    //   not running beside this one (a profiler that serialises kernels, a busy device)
constexpr unsigned kServerIdlePolls = 400000u;      // ... = half a second without a further command

__device__ __forceinline__ void mail_store(void *p, unsigned long long v) { __hip_atomic_store((env_gu64 *)p, v, GRLX_RLX_AGENT); }
__device__ __forceinline__ unsigned long long mail_load(const void *p) { return __hip_atomic_load((env_gu64 *)p, GRLX_RLX_AGENT); }
__device__ __forceinline__ void mail_setprio(unsigned p)
{
  if (p == 1) __builtin_amdgcn_s_setprio(1);
  else if (p == 2) __builtin_amdgcn_s_setprio(2);
  else if (p == 3) __builtin_amdgcn_s_setprio(3);
}
__device__ __forceinline__ unsigned long long mail_clock()
{
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

// one unit, one access
__device__ __forceinline__ void unit_store(MailUnit *p, double v, unsigned long long seq)
{
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  mail_u32x4 d;
  d.x = (unsigned)b; d.y = (unsigned)(b >> 32); d.z = (unsigned)seq; d.w = (unsigned)(seq >> 32);
  // (s_nop: a store of more than 8 bytes reads its data registers a cycle late, and the assembler does not see into this string)
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(d) : "memory");
}
// server side: unit I of a candidate, at a constant offset from the candidate's first unit (the address is computed once for the five)
template <int I, int STRIDE = 1>
__device__ __forceinline__ void unit_store_at(MailUnit *p, double v, unsigned long long seq)
{
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  mail_u32x4 d;
  d.x = (unsigned)b; d.y = (unsigned)(b >> 32); d.z = (unsigned)seq; d.w = (unsigned)(seq >> 32);
  asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1\n\ts_nop 1" ::"v"(p), "v"(d), "n"(I * STRIDE * (int)sizeof(MailUnit)) : "memory");
}
// server side: the three units of a start state, all loads in flight together, then ONE wait; true when every unit carries `seq`
// (inline assembly, waited for on the spot: nothing else is in flight in the server when it reads a start state)
template <int N>
__device__ __forceinline__ bool units_load(const MailUnit *p, unsigned long long seq, double *v)
{
  static_assert(N == 3, "");
  mail_u32x4 d[N];
  asm volatile("global_load_dwordx4 %0, %3, off sc1\n\t"
               "global_load_dwordx4 %1, %3, off offset:16 sc1\n\t"
               "global_load_dwordx4 %2, %3, off offset:32 sc1\n\t"
               "s_waitcnt vmcnt(0)"
               : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2])
               : "v"(p)
               : "memory");
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i)
  {
    ok = ok && (((unsigned long long)d[i].w << 32) | d[i].z) == seq;
    v[i] = __longlong_as_double((long long)(((unsigned long long)d[i].y << 32) | d[i].x));
  }
  return ok;
}

// rollout side: a replica's mailbox as {all mailboxes (wave-uniform), replica}.  The address is made where it is used: held as a pointer
// per lane it is a register pair for the whole launch (and a pair more for every field address the compiler derives from it ahead of
// the loops) -- registers the pass loop of rollout_served_kernel does not have.  (in_reg, grlx_policy.h, keeps the few address
// instructions at the use: the compiler would otherwise move them out of every loop again.)
struct MailRef {
  EnvMail *all;
  uint32_t r;
  __device__ __forceinline__ EnvMail *get() const { return all + in_reg(r); }
  __device__ __forceinline__ EnvMail *operator->() const { return get(); }
};
// rollout side, ONE lane of the replica's group
__device__ __forceinline__ void mail_send(EnvMail *m, unsigned long long seq, unsigned op) { mail_store(&m->cmd[seq & 3u], (seq << 8) | op); }
__device__ __forceinline__ void mail_send_reset(EnvMail *m, unsigned long long seq, const double *x)
{
  // (from the mailbox's own address with immediate offsets: three addresses of their own were three register pairs that the compiler
  //  kept for the whole launch -- registers the pass loop of rollout_served_kernel does not have)
  static_assert(offsetof(EnvMail, reset) == 2 * sizeof(MailUnit), "reset[i] is unit 2 + i of the mailbox");
  MailUnit *u = reinterpret_cast<MailUnit *>(m);
  unit_store_at<2>(u, x[0], seq);
  unit_store_at<3>(u, x[1], seq);
  unit_store_at<4>(u, x[2], seq);
  mail_send(m, seq, kMailReset);
}
__device__ __forceinline__ void mail_send(const MailRef &m, unsigned long long seq, unsigned op) { mail_send(m.get(), seq, op); }
__device__ __forceinline__ void mail_send_reset(const MailRef &m, unsigned long long seq, const double *x) { mail_send_reset(m.get(), seq, x); }

// rollout side, all 16 lanes of the replica's group: what command `seq` followed by action `a` leaves.  Lane j < 5 loads unit j (4 registers
// instead of 20), the group agrees on whether all five were the ones of `seq`, and the values are handed round.  The load is a buffer
// load the compiler schedules and waits for itself, so that it can be issued early (mail_prefetch, right after the action is chosen: one
// trip through memory, 2.3 k cycles, hidden behind the rest of the pass) and looked at late (mail_take, when the next pass starts).
template <bool BY_UNIT>            // (a tag no member uses: the layout `at` was made for, so that a reader of the other layout does not compile)
struct MailBox {
  __amdgpu_buffer_rsrc_t rs;      // all mailboxes of the launch
  unsigned at;                    // this lane's byte offset: its replica's mailbox + the unit it loads
};
template <bool BY_UNIT>
__device__ __forceinline__ MailBox<BY_UNIT> mailbox_of(const DevParams &P, int r, int j)
{
  MailBox<BY_UNIT> b;
  b.rs = __builtin_amdgcn_make_buffer_rsrc((void *)P.env_mail, 0, (int)((size_t)P.n_replicas * kEnvMailBytes), 0x00020000);
  b.at = (unsigned)r * (unsigned)kEnvMailBytes + (unsigned)offsetof(EnvMail, cand) + (unsigned)(j < kCandUnits ? j : 0) * (unsigned)((BY_UNIT ? kCandSlots : 1) * sizeof(MailUnit));
  return b;
}
template <bool BY_UNIT>
__device__ __forceinline__ mail_u32x4 mail_prefetch(const MailBox<BY_UNIT> &b, unsigned long long seq, int a)
{
  const unsigned off = BY_UNIT ? b.at + (((unsigned)seq & 1u) * (unsigned)(kCandUnits * kCandSlots) + (unsigned)a) * (unsigned)sizeof(MailUnit)
                               : b.at + (((unsigned)seq & 1u) * 3u + (unsigned)a) * (unsigned)(kCandUnits * sizeof(MailUnit));
  return __builtin_amdgcn_raw_buffer_load_b128(b.rs, off, 0, 16);         // 16 = sc1: device scope
}
template <int ENV, bool BY_UNIT>
__device__ __forceinline__ bool mail_take(const DevParams &N, const MailBox<BY_UNIT> &b, mail_u32x4 d, unsigned long long seq, int a, int g,
                                          unsigned long long gmask, double *x, double *obs, double &reward, int &terminal, uint32_t &status,
                                          unsigned long long *polled = nullptr)
{
  static_assert(ENV == GRLX_ENV_PENDULUM, "the pendulum's mailbox");
  bool ok = false;
  unsigned polls = 0;
  for (;;)
  {
    const bool mine = (((unsigned long long)d.w << 32) | d.z) == seq;
    if ((__ballot(mine) & gmask) == gmask) { ok = true; break; }
    if (++polls > (seq <= 1u ? kFirstFetchPolls : kFetchPolls)) break;
    d = mail_prefetch(b, seq, a);
  }
  if (polled) *polled += polls;
  if (!ok) return false;
  const double v = __longlong_as_double((long long)(((unsigned long long)d.y << 32) | d.x));
  const int base = g * 16;
  x[0] = lane_fetch(v, base + 0);
  x[1] = lane_fetch(v, base + 1);
  x[2] = lane_fetch(v, base + 2);
  obs[0] = lane_fetch(v, base + 3);
  obs[1] = x[1];
  reward = lane_fetch(v, base + 4);
  terminal = x[2] > N.timeout ? 1 : 0;                            // Env::observe
  if (!Env<ENV>::in_domain(x)) status |= ST_DOMAIN;             // env_step
  return true;
}
// The same take for a wave whose FOUR groups are all served and all mid-episode (the wave-uniform pass of rollout_body): the vote is over
// the whole wave -- while any group's five units are not yet those of `seq`, every lane polls again -- so the loop is one scalar branch
// and nothing around it is per lane.  A unit that carries `seq` is final, so polling a group that already had its answer reads the same
// values again: same bits as mail_take.  On running into kFetchPolls NOTHING is changed (x, obs, reward, terminal, status as they were):
// the caller leaves its loop and the general pass takes this step with mail_take, falling back per replica there.
template <int ENV, bool BY_UNIT>
__device__ __forceinline__ bool mail_take_wave(const DevParams &N, const MailBox<BY_UNIT> &b, mail_u32x4 d, unsigned long long seq, int a, int g,
                                               double *x, double *obs, double &reward, int &terminal, uint32_t &status,
                                               unsigned long long *polled = nullptr)
{
  static_assert(ENV == GRLX_ENV_PENDULUM, "the pendulum's mailbox");
  unsigned polls = 0;
  while (!__all((((unsigned long long)d.w << 32) | d.z) == seq))
  {
    if (++polls > kFetchPolls)
    {
      if (polled) *polled += polls;
      return false;
    }
    d = mail_prefetch(b, seq, a);
  }
  if (polled) *polled += polls;
  const double v = __longlong_as_double((long long)(((unsigned long long)d.y << 32) | d.x));
  const int base = g * 16;
  x[0] = lane_fetch(v, base + 0);
  x[1] = lane_fetch(v, base + 1);
  x[2] = lane_fetch(v, base + 2);
  obs[0] = lane_fetch(v, base + 3);
  obs[1] = x[1];
  reward = lane_fetch(v, base + 4);
  terminal = x[2] > N.timeout ? 1 : 0;                            // Env::observe
  if (!Env<ENV>::in_domain(x)) status |= ST_DOMAIN;             // env_step
  return true;
}
// The early take of the wave-uniform loop.  cand[n & 1][.] is stored the moment command n arrives, so while pass k + 1 (which follows
// command n) works through its table phase the answers to ALL of its possible actions are already in the mailbox: lane j < 15 of a group
// loads one unit of cand[n & 1] -- lane 5 a + u unit u of candidate a, at byte 64 u + 16 a of the buffer -- and lane 15 loads unit 0 again
// (any valid unit: it only votes).  One 16-byte load per lane, as mail_prefetch; its trip through memory hides behind the trace
// forwarding, the sums and the sampler.  Once the sampler has chosen a, mail_vote_all agrees on the tags (bounded polling, as
// mail_take_wave; on running into the bound NOTHING has changed) and mail_hand_round gives every lane the five values of candidate a.
// vmcnt(0) said in the source, for a place where nothing is in flight but the compiler cannot know it (its own wait would come later,
// behind a store, and wait for that store)
__device__ __forceinline__ void mail_nothing_in_flight() { __builtin_amdgcn_s_waitcnt(0x0F70); }
__device__ __forceinline__ mail_u32x4 mail_prefetch_all(const MailBox<true> &b, unsigned long long seq, int j)
{
  // lane j = 5 a + u loads unit u of candidate a.  (b.at already holds unit j of candidate 0 for j < 5 and unit 0 for the other lanes)
  const unsigned jj = (j >= kCandUnits && j < 3 * kCandUnits) ? (unsigned)j : 0u;
  const unsigned off = b.at + ((jj % (unsigned)kCandUnits) * (unsigned)kCandSlots + jj / (unsigned)kCandUnits) * (unsigned)sizeof(MailUnit) +
                       ((unsigned)seq & 1u) * (unsigned)(kCandUnits * kCandSlots * sizeof(MailUnit));
  return __builtin_amdgcn_raw_buffer_load_b128(b.rs, off, 0, 16);         // 16 = sc1: device scope
}
__device__ __forceinline__ bool mail_vote_all(const MailBox<true> &b, mail_u32x4 &d, unsigned long long seq, int j, unsigned long long *polled = nullptr)
{
  unsigned polls = 0;
  while (!__all((((unsigned long long)d.w << 32) | d.z) == seq))
  {
    if (++polls > kFetchPolls)
    {
      if (polled) *polled += polls;
      return false;
    }
    d = mail_prefetch_all(b, seq, j);
  }
  if (polled) *polled += polls;
  return true;
}
// (after a successful mail_vote_all; `a` is the group's: the same in its sixteen lanes, any of the three from group to group)
template <int ENV>
__device__ __forceinline__ void mail_hand_round(const DevParams &N, const mail_u32x4 &d, int a, int g, double *x, double *obs, double &reward,
                                                int &terminal, uint32_t &status)
{
  static_assert(ENV == GRLX_ENV_PENDULUM, "the pendulum's mailbox");
  const double v = __longlong_as_double((long long)(((unsigned long long)d.y << 32) | d.x));
  const int base = g * 16 + kCandUnits * a;
  x[0] = lane_fetch(v, base + 0);
  x[1] = lane_fetch(v, base + 1);
  x[2] = lane_fetch(v, base + 2);
  obs[0] = lane_fetch(v, base + 3);
  obs[1] = x[1];
  reward = lane_fetch(v, base + 4);
  terminal = x[2] > N.timeout ? 1 : 0;                            // Env::observe
  if (!Env<ENV>::in_domain(x)) status |= ST_DOMAIN;             // env_step
}

// The server: block b serves the replicas 4b .. 4b+3 of rollout wave b.  It looks TWO steps ahead: lane 16 q + 3 a + a2 (a, a2 < NA) of
// replica q holds the state after the actions (a, a2) applied to the replica's last confirmed state -- nine per replica, one instruction
// stream.  When the command "the step was taken with action a*" arrives, the three lanes (a*, .) hold what the rollout wave asks for next and
// store it at once; only then do all nine integrate the level after it, each from the state lane (a*, its a) held.  The integration is off
// the path between a command and its answer (two trips through memory), at the same number of instructions per step.
// Registers: 48 (x 2: vector + accumulation) = 96 of a SIMD's 512, beside the 416 of rollout_served_kernel (83-85 used).  The pair is bound by the
// instructions its two waves issue, so what counts here is the length of the path of one command:
//   * the constants of the dynamics are made ONCE, before the loop (Env::server_consts): literals, except the additive constant of each
//     fma(z, k1, k0) of the sine's polynomials, which is held in a vector register -- an instruction reads one scalar operand, and
//     with both constants scalar the compiler copied one into a vector register beside every use;
//   * the five units of an answer are stored from one address (unit_store_at);
//   * the handling of a command is flat (see the loop).
template <int ENV, int NA, typename SPEC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(48))) void env_server_kernel(DevParams P)
{
  static_assert(NA == 3, "sixteen lanes per replica: nine pairs of actions");
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D;
  static_assert(S == 3 && D == 2, "the pendulum's mailbox");
  const DevParams &N = SPEC::numeric(P);
  const int lane = threadIdx.x & 63;
  const int q = lane >> 4, c = lane & 15;
  const int a = c / NA, a2 = c % NA;                     // (c >= 9: idle lanes, kept in step for the shuffles)
  const bool worker = c < NA * NA;
  const int r = blockIdx.x * kReplicasPerWave + q;
  bool done = r >= P.n_replicas || (P.env_tune & 64u) != 0;   // (64: tests -- a server that is not there)
  EnvMail *m = P.env_mail + (done ? 0 : r);
  const double act = N.actions[a2];
  unsigned long long expect = 1;
  // this lane's candidate: state, observed angle and reward after (a, a2)
  double cx[S], cobs0 = 0, creward = 0;
#pragma unroll
  for (int i = 0; i < S; ++i) cx[i] = 0;
  unsigned idle = 0;
  bool seen = false;
  mail_setprio((P.env_tune >> 2) & 3u);
  const typename Env<ENV>::ServerConsts ec = Env<ENV>::server_consts();     // once: eight register pairs for the whole launch
#ifdef GRLX_ENV_SERVER_STATS
  unsigned long long t_begin = mail_clock(), t_busy = 0, n_cmd = 0, n_idle = 0, n_split = 0, n_batch = 0;
#endif
  // (tests: bits 8-23 of env_tune = the server leaves, unannounced, once it has answered that many commands of a replica -- a fetch in
  //  MID-episode then runs into its bound and the rollout wave goes on by itself from there.  Bits 24-31 = which replicas of the block it
  //  leaves: bit 24 + q stands for replica q (here q < 4: bits 24-27), 0 = all of them; the others are served to the end of the launch,
  //  so that ONE 16-lane group of a rollout wave falls back while its neighbours stay served.  A bit that names a dead slot of a ragged
  //  wave changes nothing: that slot is `done` from the start.)
  const unsigned long long quit_after = (P.env_tune >> 8) & 0xFFFFu;
  const unsigned quit_mask = P.env_tune >> 24;
  const bool leaves = quit_after != 0u && (quit_mask == 0u || ((quit_mask >> q) & 1u) != 0u);
  for (;;)
  {
    if (leaves && expect > quit_after) done = true;
    if (__all(done)) break;
    unsigned long long word = 0;
    bool ready = false;
    if (!done)
    {
      word = mail_load(&m->cmd[expect & 3u]);
      ready = (word >> 8) == expect;
      if ((word >> 8) > expect) done = true;          // the replica went on without the server (its later commands overwrote this one)
    }
    if (!__any(ready))
    {
      __builtin_amdgcn_s_sleep(1);
#ifdef GRLX_ENV_SERVER_STATS
      ++n_idle;
#endif
      if (++idle > (seen ? kServerIdlePolls : kServerStartPolls)) break;
      continue;
    }
    seen = true;
    // (`idle` is reset only by an iteration that CONSUMED a command: a reset command whose start-state units never arrive -- it cannot
    //  happen while a reset is always followed by four more commands of the launch, but nothing here relies on that -- keeps `ready`
    //  true without progress, and still runs into kServerIdlePolls)
    bool progress = false;
#ifdef GRLX_ENV_SERVER_STATS
    const unsigned long long t0 = mail_clock();
    if (!__all(ready || done)) ++n_split;
    ++n_batch;
#endif
    // (flat on purpose: every level of per-lane nesting around the integration costs a copy of the candidate per command)
    bool step = false;                       // this lane has a command to answer: a step, or a reset whose start state has arrived
    unsigned op = 0u;
    if (ready)
    {
      op = (unsigned)(word & 0xFFu);
      if (op == kMailExit)
      {
        done = true;
        progress = true;
      }
      else
        step = true;
    }
    if (rarely(__any(step && op == kMailReset)))
      if (step && op == kMailReset)
      { // a trial starts: the first level is integrated here, from the start state (every lane (., a2) the same f(start, a2));
        // the lanes (0, .) then stand for "the action taken".  (A second copy of the integration: folding both levels into one loop
        // costs registers the kernel does not have -- 102 and scratch, and with scratch the two kernels no longer share the SIMDs.)
        double x[S];
        step = units_load<3>(&m->reset[0], expect, x);      // (not there yet: the command is looked at again)
        if (step)
        {
          double obs[D];
          int terminal = 0;
          uint32_t st = 0;
#pragma unroll
          for (int i = 0; i < S; ++i) cx[i] = x[i];
          env_step_consts<ENV>(N, ec, cx, act, obs, creward, terminal, st);
          cobs0 = obs[0];
          op = 0u;
        }
      }
    if (step)
    { // the answer: what the action taken leaves, for every next action
      if (worker && a == (int)op)
      {
        // (unit by unit: the three lanes of a replica that store write 48 contiguous bytes of one 64-byte block with each instruction,
        //  where candidate by candidate their units lie 80 bytes apart.  The launch is measurably shorter so; that the three become ONE
        //  write to memory is the supposed reason, not a counted one: profiles/served_eager_answers_ab.md)
        static_assert(NA <= kCandSlots, "slot a2 of every unit is this lane's");
        constexpr bool BY_UNIT = SPEC::kCandByUnit;
        constexpr int STRIDE = BY_UNIT ? kCandSlots : 1;
        MailUnit *u;
        if constexpr (BY_UNIT) u = &m->cand.by_unit[expect & 1u][0][a2];
        else u = &m->cand.by_cand[expect & 1u][a2][0];
        unit_store_at<0, STRIDE>(u, cx[0], expect);
        unit_store_at<1, STRIDE>(u, cx[1], expect);
        unit_store_at<2, STRIDE>(u, cx[2], expect);
        unit_store_at<3, STRIDE>(u, cobs0, expect);
        unit_store_at<4, STRIDE>(u, creward, expect);
      }
      // the level after it: lane (a, a2) continues from the state the lane (action taken, a) holds
      const int src = (lane & ~15) + (int)op * NA + (worker ? a : 0);
      double x[S];
#pragma unroll
      for (int i = 0; i < S; ++i) x[i] = lane_fetch(cx[i], src);
      double obs[D];
      int terminal = 0;
      uint32_t st = 0;
#pragma unroll
      for (int i = 0; i < S; ++i) cx[i] = x[i];
      env_step_consts<ENV>(N, ec, cx, act, obs, creward, terminal, st);
      cobs0 = obs[0];
      ++expect;
      progress = true;
#ifdef GRLX_ENV_SERVER_STATS
      ++n_cmd;
#endif
    }
    if (__any(progress)) idle = 0;
    else if (++idle > kServerIdlePolls) break;
#ifdef GRLX_ENV_SERVER_STATS
    t_busy += mail_clock() - t0;
#endif
  }
#ifdef GRLX_ENV_SERVER_STATS
  if (c == 0 && r < P.n_replicas)
  {
    EnvMail *mm = P.env_mail + r;
    mm->stats[0] = mail_clock() - t_begin;
    mm->stats[1] = t_busy;
    mm->stats[2] = n_cmd;
    mm->stats[3] = n_idle;
    mm->stats[9] = n_split;
    mm->stats[10] = n_batch;
  }
#endif
}

} // namespace grlx
