/* cagym.h -- C ABI of the MI355X-native batched CollisionAvoidanceEnv (libcagym_hip.so).
 *
 * The reference (mlodel/gym-exploration-2d) has no FFI layer: its boundary is the Python
 * gym.Env object `CollisionAvoidanceEnv` (gym_collision_avoidance/envs/collision_avoidance_env.py,
 * "env.py" below).  Each entry point here cites the reference interface it replaces; the Python
 * host (gym-exploration-2d_amd/) binds them with ctypes and mirrors the gym.Env surface.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Pointers marked DEVICE are HIP device pointers (e.g.
 *    torch.Tensor.data_ptr() of a contiguous ROCm tensor); HOST pointers are ordinary memory.
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *    all work is enqueued on it, nothing inside cagym_step / cagym_rollout synchronises the host.
 *  - Every call returns 0 or a negative CAGYM_E* code; cagym_last_error() gives the message.
 *    Nothing throws across the ABI.  There is NO CPU fallback: without a HIP device
 *    cagym_create fails with CAGYM_E_NODEVICE.
 *  - A handle is not thread-safe; one handle per GPU; at most ONE call per handle in flight on the device unless a function
 *    says otherwise (calls on different streams must be ordered by the caller: several entry points keep cursors on the handle).
 *  - Layout: N worlds x M agent slots, structure-of-arrays, world-major ([N][M]).
 */
#ifndef CAGYM_H
#define CAGYM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAGYM_VERSION 112 /* 0.1.2: cagym_step_begin / cagym_step_finish, CAGYM_E_DEVICE.  cagym_ga3c_act_merge, cagym_ig_robot_inputs and
                             cagym_ig_robot_actions are backward-compatible additions under the same version. */

enum { CAGYM_OK = 0, CAGYM_E_INVALID = -1, CAGYM_E_NODEVICE = -2, CAGYM_E_HIP = -3, CAGYM_E_NOMEM = -4,
       CAGYM_E_STATE = -5, CAGYM_E_UNSUPPORTED = -6,
       CAGYM_E_DEVICE = -7 /* a kernel of an earlier launch on this handle reported an internal error (a bounded intra-workgroup wait
                              expired): the handle's device state is void; every later launching call returns this code */ };

/* policy ids: which action map / policy drives an agent (env.py:298-320) */
enum { CAGYM_POL_STATIC = 0,   /* policies/StaticPolicy.py:9-12            a = (0, 0)                      */
       CAGYM_POL_NONCOOP = 1,  /* policies/NonCooperativePolicy.py:10-13   a = (pref_speed, -heading_ego)  */
       CAGYM_POL_EXTERNAL = 2, /* raw (speed, delta_heading) from ext_actions                  */
       CAGYM_POL_LEARNING = 3, /* policies/LearningPolicy.py:11-16         a = (v_pref*u0, 4*(2*u1-1))     */
       CAGYM_POL_CARRL = 4,    /* policies/CARRLPolicy.py:5-15             11-row table, index in ext[.,0] */
       CAGYM_POL_RVO = 5,      /* policies/RVOPolicy.py:53-117             ORCA half-planes (other agents and, :56-57, the
                                  world's rectangles) + 2-D LP; needs non-degenerate rectangles, and among them
                                  cagym_set_scenarios caps the handle's max_obstacles per kernel specialisation:
                                  max_agents 4: 6, 10: 11, 20: 15, other <= 12: 9, 13..32: 16 (2*max_obstacles +
                                  max_agents - 1 half-plane slots of an LP group: 16 for max_agents 4, 32 for 10, 64
                                  otherwise; 2*max_obstacles <= 32; the obstacle-candidate lists in the LP scratch,
                                  13 B per (ego, candidate); the roll-out's LDS within 160 KB)                      */
       CAGYM_POL_GA3C = 6,     /* policies/GA3CCADRLPolicy.py:34-43        the step reads ext_actions; cagym_ga3c_act /
                                  cagym_ga3c_act_merge write these agents' rows (the host env drives them inside step
                                  once a GA3C policy is attached)                                               */
       CAGYM_POL_IGMCTS = 7 }; /* policies/ig_mcts.py:79-109               the step reads ext_actions; cagym_ig_robot_inputs ->
                                  cagym_ig_update_belief -> cagym_dmcts_plan -> cagym_ig_robot_actions write
                                  these agents' (v, omega) (the host env drives them once ig_mcts is attached)  */

/* dynamics ids (envs/dynamics/) */
enum { CAGYM_DYN_UNICYCLE = 0,    /* UnicycleDynamics.py:10-24                 */
       CAGYM_DYN_MAXTURNRATE = 1, /* UnicycleDynamicsMaxTurnRate.py:11-25      */
       CAGYM_DYN_MAXACC = 2,      /* UnicycleDynamicsMaxAcc.py:17-39           */
       CAGYM_DYN_SECONDORDER = 3, /* UnicycleSecondOrderEulerDynamics.py:12-29 */
       CAGYM_DYN_FIRSTORDER = 4 };/* FirstOrderDynamics.py:10-23               */

/* game_over rule (env.py:722-736) */
enum { CAGYM_GO_AGENT0 = 0,    /* EVALUATE_MODE && !HOMOGENEOUS_TESTING, or TRAIN_SINGLE_AGENT */
       CAGYM_GO_ALL = 1,       /* EVALUATE_MODE && HOMOGENEOUS_TESTING                         */
       CAGYM_GO_LEARNING = 2 };/* all agents with CAGYM_POL_LEARNING done                      */

/* per-agent status byte (`flags` output and state view) */
enum { CAGYM_FLAG_AT_GOAL = 1, CAGYM_FLAG_IN_COLLISION = 2, CAGYM_FLAG_RAN_OUT_OF_TIME = 4, CAGYM_FLAG_DONE = 8,
       CAGYM_FLAG_WAS_AT_GOAL = 16, CAGYM_FLAG_WAS_IN_COLLISION = 32, CAGYM_FLAG_ACTIVE = 64 };

/* Replaces the class attributes of envs/config.py read by the hot path. */
typedef struct {
    int32_t n_worlds;            /* N: worlds stepped together (one reference env instance each)            */
    int32_t max_agents;          /* M: Config.MAX_NUM_AGENTS_IN_ENVIRONMENT (config.py:70); 2..32           */
    int32_t n_scenarios;         /* S >= N: scenario pool; world w starts episode e on scenario (w+e*N)%S   */
    int32_t max_obstacles;       /* rectangles per scenario (0 = free space; env.py:492-497)                */
    int32_t game_over_mode;      /* CAGYM_GO_*                                                              */
    int32_t collide_with_static; /* Config.COLLISION_AV_W_STATIC_AGENT (config.py:52)                       */
    int32_t laserscan;           /* 1: every agent carries a LaserScanSensor (sensors/LaserScanSensor.py)   */
    int32_t device;              /* HIP device ordinal                                                      */
    double dt;                   /* Config.DT (config.py:29)                                                */
    int32_t rvo_max_neighbors;   /* RVO maxNeighbors; 0 = max_agents, as policies/RVOPolicy.py:15,25 passes it */
    int32_t reserved;            /* 0 */
} cagym_config;

#define CAGYM_EGO_WIDTH 12
/* Caller-owned DEVICE output buffers of one step.  Any pointer may be NULL (not written).
 * obs_ego columns: dist_to_goal, rel_goal.x, rel_goal.y, radius, heading_ego_frame,
 *   heading_global_frame, pos.x, pos.y, pref_speed, num_other_agents_observed, use_ppo, 0
 *   (the scalar keys of Config.STATE_INFO_DICT, config.py:104-215).
 * obs_oas: OtherAgentsStatesSensor table, rows farthest->closest (sensors/OtherAgentsStatesSensor.py:11-77).
 * For cagym_rollout every buffer has a leading [T] dimension. */
typedef struct {
    float* obs_oas;     /* [N, M, M-1, 10] f32 */
    float* obs_ego;     /* [N, M, 12]      f32 */
    float* laserscan;   /* [N, M, 16]      f32 (only when cfg.laserscan)                           */
    float* reward;      /* [N, M]          f32: _compute_rewards (env.py:502-567), all agents      */
    uint8_t* flags;     /* [N, M]          u8 : CAGYM_FLAG_* after the step (env.py:711-721)       */
    uint8_t* game_over; /* [N]             u8 : env.py:722-738                                     */
} cagym_outputs;

/* Zero-copy DEVICE views of the SoA state (for parity tests / Agent-like host views; agent.py:9-109). */
typedef struct {
    double *pos_x, *pos_y, *vel_x, *vel_y, *heading, *heading_ego, *dist_to_goal, *time_remaining, *t;
    double *goal_x, *goal_y, *radius, *pref_speed, *speed, *delta_heading, *aux0, *aux1;
    float* action;          /* [N, M, 2] last applied (speed, delta_heading), fp32 as env.py:289 */
    uint32_t* status;       /* [N, M] bits 0-7 CAGYM_FLAG_*, 8-11 policy id, 12-15 dynamics id   */
    int32_t* step_num;      /* [N, M] agent.py:186                                               */
    int32_t* n_agents;      /* [N]                                                               */
    int32_t* n_observed;    /* [N, M] num_other_agents_observed                                  */
    int32_t* episode;       /* [N] episodes started by this world (selects the scenario)         */
    uint32_t* map_bits;     /* [S, 300, 10] bit-packed occupancy rasters (Map.py:107-123) or NULL */
    /* cumulative per-world episode statistics (the payload of the multi-GPU all-gather) */
    float* stat_return;     /* [N] sum over finished episodes of agent-0 episode return          */
    int32_t* stat_episodes; /* [N] finished episodes                                             */
    int32_t* stat_steps;    /* [N] env steps in finished episodes                                */
    int32_t* stat_outcomes; /* [N, 3] agents finished at goal / in collision / timed out         */
} cagym_state_ptrs;

int cagym_version(void);

/* CollisionAvoidanceEnv.__init__ (env.py:60-160) for N worlds. */
int cagym_create(const cagym_config* cfg, void** env_out);
/* CollisionAvoidanceEnv.close (env.py:268-270). */
int cagym_destroy(void* env);
const char* cagym_last_error(void* env);

/* set_agents / _init_agents / set_static_map (env.py:387-388, 403-476, 478-500): upload the scenario
 * pool.  All pointers HOST.  agents6[S,M,6] = start_x, start_y, goal_x, goal_y, pref_speed, radius (the
 * "legacy cadrl" row of test_cases.py:1970-2014); heading0[S,M] or NULL (toward goal, agent.py:29-31);
 * policy_id / dynamics_id [S,M]; n_agents[S] or NULL (= M); coop[S,M] or NULL (1.0, agent.py:10);
 * obstacles[S,K,4] = xl, yl, xu, yu or NULL; n_obst[S].  Rasterises the obstacle maps on device. */
int cagym_set_scenarios(void* env, const double* agents6, const double* heading0, const int32_t* policy_id,
                        const int32_t* dynamics_id, const int32_t* n_agents, const double* coop,
                        const double* obstacles, const int32_t* n_obst, void* stream);

/* reset() (env.py:234-266) for the worlds whose world_mask byte is non-zero (DEVICE [N], NULL = all):
 * re-initialise agents from the world's current scenario, sense, write observations to `out`.
 * advance_episode != 0 moves the masked worlds to their next scenario first. */
int cagym_reset(void* env, const uint8_t* world_mask, int advance_episode, const cagym_outputs* out, void* stream);

/* step(actions) (env.py:162-232): _take_action -> _compute_rewards(+_check_for_collisions) -> _get_obs ->
 * _check_which_agents_done.  ext_actions DEVICE [N,M,2] f32 or NULL (all agents internal, env_utils.py:46). */
int cagym_step(void* env, const float* ext_actions, const cagym_outputs* out, void* stream);

/* cagym_step followed, in the same launch, by DummyVecEnv's auto-reset (exp/env_utils.py:29-31): a world whose
 * game_over fires restarts on its next scenario, its episode statistics are folded, and the observation written
 * for this step -- OtherAgentsStates, scalar keys and, with cfg.laserscan, the laser scan (_get_obs runs every sensor,
 * env.py:740-753) -- is the first one of the new episode (reward / flags / game_over are the terminal ones). */
int cagym_step_autoreset(void* env, const float* ext_actions, const cagym_outputs* out, void* stream);

/* step(actions) in TWO launches, for callers whose external actions come from a device policy of their own (cfg4: cagym_ga3c_act).
 * _take_action (env.py:287-340) gathers the actions of ALL agents before any agent moves, and an internal RVO policy
 * (policies/RVOPolicy.py:53-117) reads the state BEFORE the step only - so the RVO half of the step does not have to wait for the
 * external actions:
 *   cagym_step_begin   the ORCA half-planes (agents and rectangles) and linear programs of every live RVO ego on the current state;
 *                      8 bytes per agent are kept on the handle.  Enqueue it on a stream of its own, beside the policy that
 *                      produces ext_actions; it reads the state, never writes it.  A no-op for handles without RVO agents.
 *   cagym_step_finish  the rest of the step (action maps + dynamics with every action in hand, collisions, rewards, done /
 *                      game_over, observations, and - auto_reset != 0 - cagym_step_autoreset's restart).  The caller orders it
 *                      behind BOTH the begin launch and the producer of ext_actions (stream / event dependencies).
 * begin + finish produce bit for bit what cagym_step / cagym_step_autoreset produce (tests/test_split_step.py).  finish without
 * a begin since the last finish / step / reset / rollout returns CAGYM_E_STATE.  Generation-3 kernels only. */
int cagym_step_begin(void* env, void* stream);
int cagym_step_finish(void* env, const float* ext_actions, const cagym_outputs* out, int auto_reset, void* stream);

/* n_steps consecutive step() calls in ONE launch for worlds whose agents are all driven internally
 * (Static / NonCooperative / RVO): the agent records stay on chip, every step writes its outputs (laserscan
 * [T, N, M, 16] included when cfg.laserscan) to slice t of `out` ([T, ...] buffers; T = n_steps).  auto_reset != 0: a world whose game_over fires is
 * reset onto its next scenario inside the kernel (what stable-baselines' DummyVecEnv does around the
 * reference env, exp/env_utils.py:29-31) and its episode statistics are accumulated. */
int cagym_rollout(void* env, int n_steps, int auto_reset, const cagym_outputs* out, void* stream);

int cagym_get_state(void* env, cagym_state_ptrs* out);

/* The per-world episode statistics as ONE packed [N, 6] int32 table, written by one kernel: {bit pattern of the fp32 return
 * sum, finished episodes, env steps in them, agents at goal / in collision / timed out} - the 24-byte record the multi-GPU
 * all-gather carries (the reference's per-episode statistics are experiments/src/env_utils.py:41-75).
 * records: device pointer, N * 6 int32. */
int cagym_pack_episode_stats(void* env, int32_t* records, void* stream);

/* Name of the kernel instantiation this handle launches for cagym_step / cagym_step_autoreset (rollout == 0) or
 * cagym_rollout (rollout != 0), as rocprofv3 --kernel-trace prints it (bench.py reports it next to the roofline). */
int cagym_kernel_name(void* env, int rollout, int auto_reset, char* buf, int buf_len);

/* LaserScanSensor.sense (sensors/LaserScanSensor.py:27-58) on the current state -> laserscan [N,M,16]. */
int cagym_laserscan(void* env, float* laserscan, void* stream);

/* GA3CCADRLPolicy.agents_to_ga3c_cadrl_state (policies/GA3CCADRLPolicy.py:45-106) for every active agent:
 * state DEVICE [N,M,76] f32 = [id, n_others, dist_to_goal, heading_ego, pref_speed, radius, 10 x (p_prll,
 * p_orth, v_prll, v_orth, r_other, r_host+r_other, edge distance)], others sorted by (-round(d,2), p_orth),
 * the closest `max_observed` (Config.MAX_NUM_OTHER_AGENTS_OBSERVED, <= 10) kept, farthest first.  The network
 * itself (LSTM-64 + 3 x FC-256, network.py:65-98) is evaluated by the host policy on state[:, :, 1:]. */
int cagym_ga3c_state(void* env, int max_observed, float* state, void* stream);

/* NetworkVP_rnn forward pass (policies/GA3C_CADRL/network.py:65-98) + argmax + action table (network.py:8-17,
 * GA3CCADRLPolicy.find_next_action :34-43) for the B agents listed in agent_idx (flat world*M + slot), reading
 * their rows of `state` (cagym_ga3c_state).  weights: DEVICE blob of CAGYM_GA3C_NWEIGHTS floats in the order
 * lstm kernel [71,256], lstm bias, layer1 kernel [68,256], bias, layer2 kernel [256,256], bias, fullyconnected1
 * kernel [256,256], bias, logits_p kernel [256,11], bias (TensorFlow [in][out] layout).  Writes
 * ext_actions[agent] = (pref_speed * a0, a1) (DEVICE [N,M,2] f32); action_index [B] i32 and probs [B,11] f32
 * (softmax_p) are optional. */
#define CAGYM_GA3C_NWEIGHTS 170507
/* The forward kernels multiply on gfx950's 16-bit matrix cores with every fp32 operand split into two f16 halves (three matrix
 * instructions per product, fp32 accumulation: fp32-class accuracy, csrc/cagym_ga3c16.h).  The handle keeps the blob re-ordered
 * into operand fragments; that copy is made on `stream` the first time cagym_ga3c_forward / cagym_ga3c_act see a blob ADDRESS.
 * A caller that rewrites the same blob in place (training) calls cagym_ga3c_load_weights afterwards; one blob per handle is
 * cached.  CAGYM_GA3C=mfma32 / valu (environment, read per call) select the exact-fp32 kernels of rounds 2 / 1 for A/B. */
int cagym_ga3c_load_weights(void* env, const float* weights, void* stream);
int cagym_ga3c_forward(void* env, const float* weights, const float* state, const int32_t* agent_idx, int B,
                       float* ext_actions, int32_t* action_index, float* probs, void* stream);

/* GA3CCADRLPolicy.find_next_action (policies/GA3CCADRLPolicy.py:34-43) for EVERY active agent whose policy id is
 * CAGYM_POL_GA3C, in one call and without a host round trip: the agents are listed on the device, their state vectors built
 * (only theirs, as the reference does per agent), the network evaluated and (pref_speed * a0, a1) written to their rows of
 * ext_actions [N*M, 2] f32; other rows are untouched.  ONE kernel launch (round 4: a workgroup per 32 worlds lists its agents,
 * keeps their state vectors in LDS and runs the network on them); it replays from a captured HIP graph.  work: caller-owned
 * DEVICE scratch of cagym_ga3c_act_workspace_bytes(env) bytes - used (overwritten; layout private) only by the A/B kernels
 * CAGYM_GA3C=mfma32 / valu, which run the three-launch chain of rounds 2 - 3; one call per handle in flight. */
size_t cagym_ga3c_act_workspace_bytes(void* env);
int cagym_ga3c_act(void* env, const float* weights, int max_observed, void* work, float* ext_actions, void* stream);

/* cagym_ga3c_act writing the WHOLE action table actions [N*M, 2] in its one launch: every active GA3C agent gets (pref_speed * a0, a1)
 * as cagym_ga3c_act computes it, every other slot its row of ext_in [N*M, 2] (DEVICE, read-only) or (0, 0) when ext_in is NULL.  ext_in
 * must not alias actions (CAGYM_E_INVALID), so a step driven this way leaves the caller's action buffer untouched; both 8-byte aligned.
 * CAGYM_GA3C=mfma32 / valu: a device copy (or clear) of the table, then cagym_ga3c_act's chain. */
int cagym_ga3c_act_merge(void* env, const float* weights, int max_observed, void* work, const float* ext_in, float* actions,
                         void* stream);

/* ---- information-gain planner primitives (cfg 5).  All pointers DEVICE.  A visibility set is a
 * [60] u64 mask: bit i of word j <=> belief cell (i, j) (x index i, y index j; 0.5 m cells over 30x30 m). ---- */

/* ig_mcts.set_param (policies/ig_mcts.py:56-77): build the Euclidean distance field of every scenario
 * raster (edfMap.update, information_models/edfMap.py:11-12) and N belief grids at prior 1.0
 * (targetMap.__init__, information_models/targetMap.py:7-24).  Needs max_obstacles > 0. */
int cagym_ig_init(void* env, void* stream);
/* re-initialise the belief grids of the masked worlds (NULL = all) to the prior. */
int cagym_ig_reset_belief(void* env, const uint8_t* world_mask, void* stream);
/* READ-ONLY views: edf_d2 [S,300,300] u32 squared cell distances (EDF = sqrt(d2)*0.1), belief [N,60,60] f64 odds.  The belief
 * changes through cagym_ig_reset_belief / cagym_ig_update_belief only: the library keeps the per-cell mutual information of the
 * belief beside it (the reward sums of cagym_ig_mi_reward / cagym_ig_rollouts / cagym_dmcts_plan read that cache). */
int cagym_ig_get(void* env, uint32_t** edf_d2, double** belief);
/* Zero-copy DEVICE views of the team reward's per-world episode accumulators (cagym_ig_episode_boundary keeps them): running [N]
 * f64 = sum of the team reward over the steps of the episode in progress, sum [N] f64 = sum of the finished episodes' returns,
 * last [N] f64 = return of the last finished episode, episodes [N] i32 = finished episodes.  Owned by the handle, allocated with
 * the IG state, zeroed by every cagym_ig_init.  Any pointer may be NULL. */
int cagym_ig_get_episode_stats(void* env, double** running, double** sum, double** last, int32_t** episodes);
/* targetMap.getVisibleCells (targetMap.py:43-84) for Q poses (x, y, phi) of worlds world[q]. */
int cagym_ig_visible_cells(void* env, const double* poses, const int32_t* world, int Q, double fov_rad,
                           double range, uint64_t* masks, void* stream);
/* targetMap.update (targetMap.py:86-128), frame='global': poses [N,P,3] applied in order, n_poses [N] or
 * NULL (= P), detections [N,P,Dmax,2] global positions, n_det [N,P]; observed [N,60] = union of the visible
 * sets (NULL to skip).  ig_mcts.update_belief (ig_mcts.py:117-133). */
int cagym_ig_update_belief(void* env, const double* poses, const int32_t* n_poses, const double* detections,
                           const int32_t* n_det, int P, int Dmax, double fov_rad, double range, uint64_t* observed,
                           void* stream);
/* targetMap.get_reward_from_cells (targetMap.py:130-143): reward[q] = sum of cell MI over masks[q]. */
int cagym_ig_mi_reward(void* env, const uint64_t* masks, const int32_t* world, int Q, double* reward, void* stream);
/* ig_mcts.get_next_pose (ig_mcts.py:154-183): xdt Euler sub-steps of dt; feasible[q] = 0 where the
 * reference returns None (next[q] is then the input pose). */
int cagym_ig_next_pose(void* env, const double* poses, const double* actions, const int32_t* world,
                       const double* radius, int Q, int xdt, double dt, double* next, uint8_t* feasible, void* stream);
/* Tree._simulate (policies/pydecmcts/DecMCTS.py:233-271) x nsims per query: n_steps[q] uniformly random
 * motion primitives (ig_mcts.mcts_avail_actions :247-253; counter-based RNG on (seed, q, sim, step)) from
 * pose0[q] with already-observed set observed0[q]; reward = MI(observed minus exclude[q]) (mcts_reward :234-241).
 * rewards [Q,nsims]; actions [Q,nsims,max_steps] primitive index 0..8 or 255 (infeasible draw; may be NULL);
 * final_pose [Q,nsims,3] (may be NULL); observed_out [Q,nsims,60] = cells observed along each roll-out including
 * observed0, before exclusion (may be NULL) -- the set a robot communicates to its team (MCTS_state.obsvd_cells). */
int cagym_ig_rollouts(void* env, const double* pose0, const uint64_t* observed0, const uint64_t* exclude,
                      const int32_t* world, const int32_t* n_steps, const double* radius, int Q, int nsims,
                      int max_steps, int xdt, double dt, double fov_rad, double range, uint64_t seed,
                      double* rewards, uint8_t* actions, double* final_pose, uint64_t* observed_out, void* stream);

/* OccupancyGridSensor.sense (sensors/OccupancyGridSensor.py:70-98) for every agent of the current
 * state: grid DEVICE [N, M, 60, 60] u8 (0 / 1), the 'local_grid' observation: the obstacle raster rotated into the
 * agent's heading (cv2.warpAffine restated, bilinear, zero border) and cropped around the agent.  Needs
 * max_obstacles > 0.  PARITY UNPINNED: OpenCV is not available to check the restatement against. */
int cagym_occupancy_grid(void* env, uint8_t* grid, void* stream);

/* ---- on-device scenario generation ---------------------------------------------------
 * train_agents_random_positions (test_cases.py:1362-1463) for every scenario of the pool, one lane per
 * scenario: per agent draw start x, y and goal x, y ~ U(-side, side) (four draws per attempt, in that order)
 * until the start is >= min_sep from every earlier start, the goal >= min_sep from every earlier goal
 * (is_pose_valid, test_cases.py:129-133) and |goal - start| >= min_travel; radius / pref_speed / cooperation
 * coefficient constant (:1364-1365, :1426).  Agents per scenario ~ U{n_min..n_max} (random.randint(2, n) when
 * unseeded, n when seeded, :1367-1372).  Agent 0 gets (ego_policy, ego_dynamics); every other agent policy_b
 * with probability p_b else policy_a (random.choice of two = 0.5, :1417; 0.2 in :1352-1355) and other_dynamics.
 * Random numbers: counter-based (splitmix64 finaliser on (seed, scenario, draw)), NOT numpy's global MT19937
 * stream, so agreement with the reference is distributional; the CPU oracle uses the same generator and agrees
 * bit for bit.  max_tries bounds the rejection loop (the last draw is kept; *n_failed counts such agents). */
typedef struct cagym_gen_params {
    uint64_t seed;
    int32_t n_min, n_max;
    int32_t ego_policy, ego_dynamics;
    int32_t policy_a, policy_b, other_dynamics;
    int32_t max_tries;
    double p_b;
    double side, min_travel, min_sep, radius, pref_speed, coop;
} cagym_gen_params;
int cagym_generate_scenarios(void* env, const cagym_gen_params* params, int32_t* n_failed_host, void* stream);

/* zero-copy DEVICE views of the scenario pool (parity tests, dataset export) */
typedef struct cagym_scenario_ptrs {
    const double* agents6;    /* [S, M, 6] */
    const int32_t* policy;    /* [S, M]    */
    const int32_t* dynamics;  /* [S, M]    */
    const int32_t* n_agents;  /* [S]       */
    const double* coop;       /* [S, M]    */
} cagym_scenario_ptrs;
int cagym_get_scenarios(void* env, cagym_scenario_ptrs* out);

/* ---- on-device samplers of the reference's training scenarios (tc.py:1192-1463, 2359-2572) -------------------
 * cagym_generate_reference_scenarios fills every scenario of the pool with one sampler of test_cases.py, one lane per scenario,
 * on the counter-based generator of cagym_generate_scenarios: u(k) = U[0,1) draw k of the scenario's stream (seed, scenario),
 * U(lo, hi) = lo + (hi - lo) * u(k).  NOT numpy's / random's MT19937 streams: agreement with the reference is distributional.
 * nmax = max(number_of_agents, 2); a count draw  c(lo, hi) = lo + (int)(u(k) * (hi - lo + 1)), clamped, is still made (and
 * ignored) when fixed_count != 0, which takes hi (the reference's seeded branch, tc.py:1206-1209).  Distances are
 * sqrt(dx*dx + dy*dy) in fp64; every rejection loop stops after max_tries attempts, keeps its last draw and adds the agents
 * (a pair counts 2) or rectangles it placed that way to *n_failed.  Policies of the non-ego agents, per agent in slot order:
 * u(k) < p_b ? policy_b : policy_a, with (policy_a, policy_b, p_b) = each kind's rule below or, override_policies != 0, the
 * caller's.  Rows of slots >= n_agents: (0, 0, 0, 0, 1, 0.5), Static, Unicycle.  heading: toward the goal (agent.py:29-31).
 *   SWAP_CIRCLE (train_agents_swap_circle, tc.py:1192-1282): u0: n = c(2, nmax); n_agents = 2 * (n / 2).  Per pair p:
 *     distance = U(4, 8), angle = U(-pi, pi) (2 draws per attempt), s = distance * (cos, sin)(angle); slot 2p starts at -s
 *     with goal s, slot 2p+1 the reverse; pairs p > 0 retry until both s and -s are >= 1.5 m from every earlier start
 *     (is_pose_valid, :129-133).  Then one policy draw per slot 1..n_agents-1.  Rule: NonCooperative with p 0.2 else RVO
 *     (uniform > 0.8, :1247-1250); coop 0.5 (ego 1.0); ego dynamics UnicycleDynamicsMaxAcc when ego_policy is GA3C.
 *   PAIRWISE_SWAP (train_agents_pairwise_swap, :1283-1364): u0: n = c(2, nmax); n positions ~ U(-7.5, 7.5)^2 (2 draws per
 *     attempt), each after the first >= 2.0 m from the earlier ones; Fisher-Yates shuffle as random.shuffle (i = n-1 .. 1:
 *     j = (int)(u(k) * (i + 1)), swap i, j); slots 2p / 2p+1 swap positions p's pair; n_agents = 2 * (n / 2).  Policy draws,
 *     rule, coop and ego dynamics as SWAP_CIRCLE.
 *   RANDOM_POSITIONS (:1365-1463): exactly cagym_generate_scenarios with n_min = 2 (nmax when fixed_count), n_max = nmax,
 *     side 7.5, min_travel 4, min_sep 1.5, radius 0.5, pref_speed 1, coop 0.5, ego dynamics as SWAP_CIRCLE; its draws are
 *     keyed and ordered as there, so both entries give bit-identical pools.  Rule: RVO / NonCooperative at p 0.5 (:1417).
 *   STAGE_1 / STAGE_2 (train_stage_1 :2359-2463 / train_stage_2 :2464-2572): u0: n_obst = c(lo, hi).  Per
 *     rectangle: u < 0.5 square of side U(1, 3) / U(1, 2), else wall wx = U(1, 4), wy = wx > 2 ? U(1, 2) : U(3, 4); then per
 *     attempt the upper corner (xu, yu) ~ U(-4, 6)^2 / U(-8, 10)^2, (xl, yl) = (xu, yu) - size, until no overlap with an earlier
 *     rectangle (is_shape_valid, :150-170: xl' >= xu || xl >= xu' || yu' <= yl || yu <= yl').  Ego: distance U(6, 8) /
 *     U(8, 10), angle U(-pi, pi), start s, goal -s, both clear of every rectangle (is_pose_valid_with_obstacles, :135-148:
 *     x >= xu + 1 || y >= yu + 1 || x <= xl - 1 || y <= yl - 1).  Then u: others = c(1, max(number_of_agents - 1, 1)),
 *     each placed as the ego and also >= 1.5 m from every earlier start and goal.  Then one policy draw per other agent.
 *     Rule: every other agent RVO (p_b = 0: other_agents_policy with no mix); coop 1.0; dynamics as given (the reference's
 *     defaults are FirstOrder for the ego, Unicycle for the others).  [lo, hi] is the reference's range, (0, 4) / (2, 10),
 *     narrowed by the caller's bounds: lo = max(ref, n_obst_min), hi = min(ref, n_obst_max), a bound < 0 being none - so in
 *     a mixture n_obst_max caps stage 2 without touching stage 1.  Rectangles: obstacles [S, max_obstacles, 4] = (xl, yl, xu, yu), zero beyond n_obst; their
 *     RVO prep rows (as cagym_set_scenarios computes them, bit for bit) and rasters are built on the device.
 * kinds_mask: bit (1 << CAGYM_GEN_*) per kind; with more than one bit every scenario draws its kind uniformly among them
 * (the np.random.randint stage of _init_agents, env.py:432-438) from a stream of its own, u(seed ^ 0xD1B54A32D192ED03, s, 0),
 * so a single kind draws nothing for it.  Refused (CAGYM_E_INVALID): an empty or unknown mask, nmax > max_agents, n_obst_max above the
 * handle's max_obstacles or below n_obst_min, a stage kind of the mask whose hi exceeds max_obstacles (it is never clamped:
 * capping it, e.g. to 6 for RVO agents at max_agents 4, is the caller's choice) or whose [lo, hi] is empty, ids out of range, max_tries < 1, p_b outside [0, 1].  With RVO agents possible among rectangles the
 * handle's max_obstacles is checked as cagym_set_scenarios checks it (same codes and messages).  A refused call leaves the
 * handle as it was; an accepted one commits the handle state as cagym_set_scenarios does (IG robot counts: unknown). */
enum { CAGYM_GEN_SWAP_CIRCLE = 0, CAGYM_GEN_PAIRWISE_SWAP = 1, CAGYM_GEN_RANDOM_POSITIONS = 2, CAGYM_GEN_STAGE_1 = 3,
       CAGYM_GEN_STAGE_2 = 4, CAGYM_GEN_NKINDS = 5 };
typedef struct cagym_gen2_params {
    uint64_t seed;
    uint32_t kinds_mask;
    int32_t number_of_agents, fixed_count;
    int32_t ego_policy, ego_dynamics;
    int32_t override_policies, policy_a, policy_b, other_dynamics;
    int32_t n_obst_min, n_obst_max; /* bounds on the stage kinds' rectangle counts; < 0: none (the reference's range) */
    int32_t max_tries;
    double p_b;
} cagym_gen2_params;
int cagym_generate_reference_scenarios(void* env, const cagym_gen2_params* params, int32_t* n_failed_host, void* stream);

/* zero-copy DEVICE views of the pool's rectangles: obst [S, max_obstacles, 4] (xl, yl, xu, yu), n_obst [S]; both NULL when
 * max_obstacles is 0 */
int cagym_get_obstacles(void* env, const double** obst, const int32_t** n_obst);

/* ---- Dec-MCTS planning step on the device ------------------------------------------------
 * ig_mcts.find_next_action for every IG robot of every world (ig_mcts.py:79-109) with the tree of
 * pydecmcts/DecMCTS.py:92-360 kept on the device: per cycle and robot, Ntree times { sample one communicated
 * plan per robot listened to, UCT selection, expansion by the feasible motion primitives, Nsims random roll-outs
 * to the horizon, discounted back-propagation, top-comm_n action distribution (q = mu^2) }, then publish.  One
 * workgroup per world; same generator keys, summation orders and tie rules as the host planner
 * gym-exploration-2d_amd/dmcts.py, whose decisions it reproduces.  poses DEVICE [N,R,3] (x, y, heading) of the
 * IG robots; workspace DEVICE, caller-owned, cagym_dmcts_workspace_bytes() bytes, holds the trees and the plans
 * the robots communicated (kept across calls like policy.best_paths; reset_comms != 0 forgets them, e.g. at an
 * episode start); call_base = number of tree grows requested by earlier calls with this seed (keys the random
 * streams).  Outputs DEVICE: actions [N,R,2] = (v, omega) of the first step of each robot's best path,
 * paths [N,R,8] primitive indices of that path (254 = infeasible draw, 255 = none), stats [N,R,3] = root mu,
 * root N, node count (may be NULL).  Limits: n_robots <= 8, horizon <= 8, Nsims <= 32, comm_n <= 8.
 * parallel_agents selects the mode of ig_mcts.set_param(..., parallelize_agents) (collision_avoidance_env.py:342-379):
 * 0 sequential (within a cycle, robot k hears what robots j < k published in that cycle; one workgroup per world),
 * 1 agent-parallel (every robot of a cycle hears the publications as they stood when the cycle started; one workgroup
 * per world and robot, one launch per cycle); any other value is refused (CAGYM_E_INVALID).  Generator keys, call_base
 * and everything else are the same in both modes.  Mode 1 needs the larger workspace cagym_dmcts_workspace_bytes()
 * reports for it (a second publication buffer); mode 0's size is unchanged.  The published plans are kept in the same
 * place in both modes, so the mode may change between calls on one workspace without reset_comms; reset_comms clears
 * the publications of the mode of the call. */
typedef struct cagym_dmcts_params {
    int32_t n_robots, Ntree, Nsims, horizon, Ncycles, comm_n, xdt, reset_comms;
    uint32_t call_base, parallel_agents;
    double c_p, gamma, radius, dt, fov_rad, range;
    uint64_t seed;
} cagym_dmcts_params;
size_t cagym_dmcts_workspace_bytes(int n_worlds, const cagym_dmcts_params* params);

/* The env's IG robots: in every world the active slots whose policy id is CAGYM_POL_IGMCTS, in slot order.  Both calls need every
 * scenario of the pool to hold exactly n_robots of them (counted by cagym_set_scenarios): CAGYM_E_INVALID otherwise, and CAGYM_E_STATE
 * after a cagym_generate_scenarios whose policies include CAGYM_POL_IGMCTS (the count is random there).  One wave per world.
 * cagym_ig_robot_inputs: the inputs of ig_mcts.update_belief (policies/ig_mcts.py:117-152) on the current state: poses [N,R,3] f64
 *   = (x, y, heading); the reference's detector emulation on each robot's OtherAgentsStates rows obs_oas [N,M,M-1,10] f32 (as the last
 *   step / reset wrote them): a row is a target when column 9 == 1.0 (a static agent) and sqrt(r0^2 + r1^2) <= detect_range, in fp32
 *   like the table (the FOV test is always true, SURVEY Q24, and left out); detections [N,R,M-1,2] f64 = row[0:2] + pose[0:2] in row
 *   order (farthest first), n_det [N,R] i32 - the layout cagym_ig_update_belief takes (P = R, Dmax = M-1).
 * cagym_ig_robot_actions: the planner's (v, omega) [N,R,2] f64 (cagym_dmcts_plan) into the robots' rows of actions [N*M,2] f32
 *   (round to nearest); other rows are untouched. */
int cagym_ig_robot_inputs(void* env, int n_robots, double detect_range, const float* obs_oas, double* poses, double* detections,
                          int32_t* n_det, void* stream);
int cagym_ig_robot_actions(void* env, int n_robots, const double* planner_actions, float* actions, void* stream);
int cagym_dmcts_plan(void* env, const cagym_dmcts_params* params, const double* poses, void* workspace,
                     size_t workspace_bytes, double* actions, uint8_t* paths, double* stats, void* stream);

/* The episode boundary of the IG team, per world: ONE launch (one workgroup per world) on `stream`, to be enqueued behind the step
 * (cagym_step_autoreset) that ended the episodes.  team_reward DEVICE [N] f64 (cagym_ig_mi_reward of this step's observation) or
 * NULL; restart_mask DEVICE [N] u8 or NULL - in a stepping loop the game_over output the step just wrote; workspace: the planner's
 * (cagym_dmcts_plan), params: the planner's (n_robots, Ntree, Ncycles and parallel_agents locate the publications; the rest is
 * not read).  For every world w, in this order:
 *   running[w] += team_reward[w]                       (fp64, in step order; skipped when team_reward is NULL)
 *   if restart_mask[w]:
 *     with CAGYM_IG_EPISODE_FOLD: sum[w] += running[w], last[w] = running[w], episodes[w] += 1  (the terminal step's reward
 *       belongs to the episode that ends); without it (a manual restart) they are left alone;
 *     running[w] = 0;
 *     the world's belief returns to the prior (the doubles of cagym_ig_reset_belief) - the next cagym_ig_update_belief is the
 *       first observation of the new episode, on the distance field of the world's new scenario;
 *     its n_robots communicated plans are forgotten: its robots hear nothing in cycle 0 of the next cagym_dmcts_plan, in
 *       either mode, a mode switch included (a workspace sized for mode 1 has the second publication buffer cleared too).
 * Nothing of a world that is not masked is touched except running[w].  A NULL mask restarts nothing: the call only accumulates.
 * CAGYM_IG_EPISODE_PLANS_ONLY: the masked worlds only lose their communicated plans (what reset_comms does to all worlds, at
 * once instead of at the next plan); beliefs and all four accumulators stay, team_reward is not read.
 * Nothing else of the planner survives a planning step (trees, counters and distributions are rebuilt by cycle 0), and the
 * generator keys keep running on call_base.  Errors as cagym_dmcts_plan: CAGYM_E_STATE before cagym_ig_init, CAGYM_E_INVALID for
 * a NULL params / workspace, n_robots, Ntree or Ncycles out of range, parallel_agents > 1, unknown flags, or a workspace smaller
 * than cagym_dmcts_workspace_bytes(n_worlds, params). */
enum { CAGYM_IG_EPISODE_FOLD = 1, CAGYM_IG_EPISODE_PLANS_ONLY = 2 };
int cagym_ig_episode_boundary(void* env, const cagym_dmcts_params* params, const double* team_reward, const uint8_t* restart_mask,
                              uint32_t flags, void* workspace, size_t workspace_bytes, void* stream);

/* ---- The one-step greedy information-gain policy (policies/ig_greedy.py:64-94) for every IG robot of every world -------------
 * ONE launch, no host synchronisation.  poses DEVICE [N,R,3] (x, y, heading; cagym_ig_robot_inputs writes this layout).  Per robot
 * and candidate c = 3 a + b = (v[a], w[b]), in this order (the reference: v = {0, 2, 4}, w = {-pi, 0, pi}, ig_greedy.py:65-68):
 *   next = pose + (v cos(heading), v sin(heading), w) dt    (one Euler step, the arithmetic of cagym_ig_next_pose's sub-step);
 *   feasible <=> EDF(next) > radius + 0.1 on the distance field of the world's current scenario, for v = 0 as well;
 *   mi[c] = sum of cell MI over getVisibleCells(next) on the world's current belief; an infeasible candidate gets -1.0 (cell MI is
 *   never negative).  The first candidate with strictly the largest mi wins (the running maximum starts at -1).
 * Outputs DEVICE: actions [N,R,2] f64 = the winner's (v, w), choice [N,R] u8 = its index, mi [N,R,9] f64 (may be NULL),
 * claimed [N,60] u64 (may be NULL; see coordinate).  Deviations from the reference: a candidate whose next cell
 * lies outside the 300 x 300 raster is infeasible (the reference wraps a negative index and raises beyond 299); with no feasible
 * candidate choice = 255 and the action is (0, 0) (the reference returns the scalar -1).
 * coordinate = 0: every robot on its own, as in the reference; one workgroup per (world, robot); claimed is written as the empty set.
 * coordinate = 1 (not in the reference, whose robots each own a map; here a world's robots share one belief): the robots of a
 *   world go in slot order with a claimed set that starts empty; robot k's mi[c] sums over visible(next_c) & ~claimed (the set
 *   difference of mcts_reward, ig_mcts.py:234-241), and after its choice claimed |= visible(next_best); a robot with choice 255
 *   claims nothing; claimed out is the final set.  Robot 0's results are those of coordinate = 0.  One workgroup per world.
 * The masks are those of cagym_ig_visible_cells and every mi[c] is, bit for bit, what cagym_ig_mi_reward returns for the same mask
 * (after & ~claimed); the same call twice writes identical bytes.
 * Errors: CAGYM_E_STATE before cagym_ig_init; CAGYM_E_INVALID for a NULL params / poses / actions / choice, n_robots outside 1..8,
 * coordinate outside {0, 1}, a non-finite or non-positive dt, fov_rad or range, a negative or non-finite radius, a non-finite
 * candidate; CAGYM_E_DEVICE as every launching entry. */
typedef struct cagym_ig_greedy_params {
    int32_t n_robots;   /* 1..8, as cagym_dmcts_plan */
    int32_t coordinate; /* 0: every robot on its own (the reference); 1: sequential team allocation */
    double dt, radius, fov_rad, range;
    double v[3], w[3];
} cagym_ig_greedy_params;
int cagym_ig_greedy_plan(void* env, const cagym_ig_greedy_params* params, const double* poses, double* actions, uint8_t* choice,
                         double* mi, uint64_t* claimed, void* stream);

/* ---- The learner's end of a step: restart, robot inputs, belief update, team reward, accumulators and belief windows, fused ----
 * For an exploration policy that is none of the built-in planners: it moves the CAGYM_POL_IGMCTS robots through the step's action
 * table and calls this behind every step or reset.  ONE launch on `stream` (one workgroup of 256 threads per world), no host
 * synchronisation, no atomics, barriers only.  params: cagym_ig_observe_params, defined in include/cagym_ig_observe.h (n_robots
 * 1..8, window = G, rotate, flags, detect_range, fov_rad, range).  obs_oas DEVICE [N,M,M-1,10] f32: the table the step or reset just
 * wrote.  restart_mask DEVICE [N] u8 or NULL - in a stepping loop the game_over output of the auto-resetting step.  Outputs, DEVICE,
 * each may be NULL: team_reward [N] f64, gain [N] f64, observed [N,60] u64, belief_window [N,R,3,G,G] f32.
 * For every world w, in this order:
 *   restarted = restart_mask && restart_mask[w].  With CAGYM_IG_OBSERVE_ONLY_RESTARTED a world that is not restarted is skipped:
 *     nothing of it is read or written (a manual restart of some worlds).
 *   if restarted: with CAGYM_IG_EPISODE_FOLD sum[w] += running[w], last[w] = running[w], episodes[w] += 1 (the accumulators of
 *     cagym_ig_get_episode_stats); running[w] = 0; belief and MI cache return to the prior, as cagym_ig_reset_belief leaves them.
 *   poses and detections of the world's n_robots robots as cagym_ig_robot_inputs computes them (kept on chip);
 *   the belief update of cagym_ig_update_belief with those poses in slot order (P = n_robots); the union of the visible cells goes
 *     to observed, and the MI cache is refreshed on that union;
 *   r = the MI sum over the union on the updated belief - bit for bit what cagym_ig_mi_reward returns for (observed[w], w);
 *   running[w] += r; gain[w] = r; team_reward[w] = restarted ? 0 : r  (the first observation of a new episode counts toward that
 *     episode's return; it is no reward for the action that ended the old one);
 *   belief_window[w, k] for robot k at pose (px, py, heading): out cell (a, b), a forward, b left (b fastest in memory), cell size
 *     c = 0.5; ex = (a - G/2 + 0.5) c, ey = (b - G/2 + 0.5) c; (s, cs) = (sin, cos)(heading) with rotate = 1, else (0, 1);
 *     qx = px + cs ex - s ey, qy = py + s ex + cs ey (fp64, separate products and sums in this order); belief cell
 *     i = floor((qx + 15) / c), j = floor((qy + 15) / c) (getCellsFromPose).  Inside 0..59 on both axes: channel 0 =
 *     (float)(odds / (odds + 1)) of belief[w, j, i], channel 1 = (float) that cell's cached MI, channel 2 = 1; outside: 0, 0, 0.
 * Belief, observed and gain are those of the chain cagym_ig_reset_belief(mask) -> cagym_ig_robot_inputs -> cagym_ig_update_belief
 * -> cagym_ig_mi_reward, bit for bit.
 * Errors: CAGYM_E_STATE before cagym_ig_init; CAGYM_E_INVALID for a NULL params / obs_oas, n_robots outside 1..8, window odd or
 * outside 4..64, rotate outside {0, 1}, unknown flags, a non-finite or non-positive fov_rad, range or detect_range; the robot-count
 * errors of cagym_ig_robot_inputs; CAGYM_E_DEVICE as every launching entry.  A refused call leaves the handle untouched. */
enum { CAGYM_IG_OBSERVE_ONLY_RESTARTED = 4 }; /* beside CAGYM_IG_EPISODE_FOLD = 1 in cagym_ig_observe_params.flags */
typedef struct cagym_ig_observe_params cagym_ig_observe_params;
int cagym_ig_observe(void* env, const cagym_ig_observe_params* params, const float* obs_oas, const uint8_t* restart_mask,
                     double* team_reward, double* gain, uint64_t* observed, float* belief_window, void* stream);

/* ---- The learner's second image: obstacle clearance, other agents and the cells seen in this update, in the belief window's frame --
 * The belief window of cagym_ig_observe shows the TARGET belief; the planners the learner is compared with also use the distance
 * field (they reject a motion whose EDF(next) <= radius + 0.1 and cast their view cones through it).  This call writes, for the same
 * robots on the same G x G sample points, what the belief window does not hold.  ONE launch on `stream` (one workgroup of 256 threads
 * per world), to be enqueued directly behind cagym_ig_observe; no host synchronisation, no atomics, barriers only; it changes nothing
 * of the handle.  params: cagym_ig_context_params, defined in include/cagym_ig_context.h (n_robots 1..8, window = G, rotate, flags,
 * clear_max).  observed DEVICE [N,60] u64 or NULL: the union cagym_ig_observe just wrote.  world_mask DEVICE [N] u8 or NULL: with
 * CAGYM_IG_CONTEXT_ONLY_MASKED a world whose mask byte is 0 (every world, for a NULL mask) is skipped - nothing of it is read or
 * written; without the flag the mask is not looked at.  context_window DEVICE [N,R,3,G,G] f32.
 * For robot k of world w (the active CAGYM_POL_IGMCTS slots in slot order) at pose (px, py, heading) and out cell (a, b), a forward,
 * b left (b fastest in memory): the sample (qx, qy), the belief cell (i, j) and (s, cs) are EXACTLY those of belief_window above, and
 * inside <=> 0 <= i, j < 60.
 *   channel 0, clearance: inside: (float)(fmin(EDF(qx, qy), clear_max) / clear_max), fp64 until the conversion, EDF the value the
 *     planners' clearance test reads from the field of the world's CURRENT scenario slot (w + episode[w] * N) % S, row = y, column = x;
 *     outside: 0.
 *   channel 1, agents: for every ACTIVE slot t of the world other than robot k's own whose policy is not CAGYM_POL_STATIC (the targets
 *     stay hidden): dx = px_t - px, dy = py_t - py, fx = cs dx + s dy, fy = cs dy - s dx (fp64, separate products and sums in this
 *     order), a_t = (int)floor(fx * 2.0) + G/2, b_t = (int)floor(fy * 2.0) + G/2; with both in 0..G-1 cell (a_t, b_t) takes
 *     max(value, v), v = 1.0 for a CAGYM_POL_IGMCTS slot (a teammate), 0.5 for any other.  Every other cell is 0.  NOT masked by inside.
 *   channel 2, seen now: 1 where inside and bit i of observed[w][j] is set, else 0; a NULL observed gives 0 everywhere.
 * Errors: CAGYM_E_STATE before cagym_ig_init; CAGYM_E_INVALID for a NULL params / context_window, n_robots outside 1..8, window odd
 * or outside 4..64, rotate outside {0, 1}, unknown flags, a non-finite or non-positive clear_max; the robot-count errors of
 * cagym_ig_robot_inputs; CAGYM_E_DEVICE as every launching entry.  A refused call touches nothing. */
enum { CAGYM_IG_CONTEXT_ONLY_MASKED = 1 }; /* cagym_ig_context_params.flags */
typedef struct cagym_ig_context_params cagym_ig_context_params;
int cagym_ig_context_window(void* env, const cagym_ig_context_params* params, const uint64_t* observed, const uint8_t* world_mask,
                            float* context_window, void* stream);

/* ---- Goal actions for the learner's robots: geodesic distance fields on the belief grid and a controller that descends them -------
 * A learner may choose a PLACE for a robot - a world point, or a cell of the belief window it is handed - instead of a (v, omega)
 * per step.  Three launches on `stream`, no host synchronisation, no global atomics, barriers only.  params of all three:
 * cagym_ig_goal_params, defined in include/cagym_ig_goals.h (n_robots = R 1..8, window = G, rotate, flags = 0, radius, v_max, w_max,
 * align_tol, goal_tol, dt); every call validates the whole block.  The robots of world w are its active CAGYM_POL_IGMCTS slots in
 * slot order; cells are those of the belief: i = floor((x + 15) / 0.5), j likewise of y, inside <=> both in 0..59.
 *
 * cagym_ig_geodesic: one workgroup of 256 threads per (world, robot); mask DEVICE [N,R] u8 or NULL (= every robot): a robot whose
 * byte is 0 is skipped, nothing of it is read or written.  Exactly one of goals_xy DEVICE [N,R,2] f64 (world metres) and goals_ab
 * DEVICE [N,R,2] i32 is non-NULL; a cell (a, b) of the robot's belief window becomes its sample point (qx, qy) of cagym_ig_observe
 * above, on the pose the state holds now.  Outputs, DEVICE: goal_xy [N,R,2] f64 the point used; active [N,R] u8 = the point is
 * finite and its cell (si, sj) inside; field [N,R,60,60] f32 indexed [j, i]; sweeps [N,R] i32 or NULL, the relaxation sweeps run.
 *   free[j, i] <=> sqrt((double)d2[5 j + 2][5 i + 2]) * 0.1 > radius + 0.1 on the field of the world's CURRENT scenario slot (the
 *     value the planners' clearance test reads at the cell's centre), or (i, j) is the source cell.
 *   field[sj, si] = 0; every other free cell holds min over its allowed neighbours u of fl32(field[u] + cost), cost 0.5f for an
 *     orthogonal and (float)(0.5 * sqrt(2.0)) for a diagonal neighbour, a diagonal allowed only when both orthogonal cells it passes
 *     between are free; blocked and unreached cells hold +inf.  The fixed point is unique (fp32 addition is monotone, costs are
 *     positive): it is a Dijkstra's result with the same additions, bit for bit.  active = 0 gives an all-inf row.
 *
 * cagym_ig_goal_actions: before the step.  For every robot with active != 0 its row of actions [N,M,2] f32 (8-byte aligned) becomes
 * ((float)v, (float)omega); every other row stays the caller's.  fp64, separate operations: (x, y, heading) the robot's pose, (ci, cj)
 * its cell, dist = sqrt(dx dx + dy dy) to the goal point.
 *   (0, 0) when the own cell is outside, when dist <= goal_tol, or when no candidate below exists.
 *   aim = the goal point when the own cell is the goal's; else the centre of the neighbour cell with the smallest key
 *     fl32(field[n] + cost(n)) among E, N, W, S, NE, NW, SW, SE (E = +x, N = +y; the first of equal keys wins) whose field value is
 *     finite and, for a diagonal while the own cell's value is finite, whose two orthogonal neighbours' values are finite too.
 *   err = wrap(atan2(ay - y, ax - x) - heading), wrap(a) = fmod(a + pi, 2 pi) made non-negative, - pi; omega = clamp(err / dt, +-w_max);
 *   atan2 is fdlibm's, evaluated as separate fp64 operations in a fixed order (ig.atan2_spec returns the same double bit for bit);
 *   rem = err - omega dt; v = 0 when |rem| > align_tol, else v_max, or fmin(v_max, dist / dt) when the aim is the goal point.
 *   choice DEVICE [N,R] u8 or NULL: what every robot aims at - 0..7 the neighbour in candidate order, 8 the goal point, 255 nothing
 *   (no active goal, or one of the (0, 0) cases).
 *
 * cagym_ig_goal_status: behind the step and cagym_ig_observe.  restart_mask DEVICE [N] u8 or NULL: the robots of a world whose byte
 * is set get active = 0.  Then for every robot goal_distance [N,R] f32 = the field at its own cell (+inf when inactive or outside) and
 * goal_reached [N,R] u8 = active and sqrt(dx dx + dy dy) <= goal_tol.
 *
 * Errors, all three, before the handle is touched: CAGYM_E_STATE before cagym_ig_init; CAGYM_E_INVALID for a NULL params, field,
 * goal_xy or active (or actions; goal_distance, goal_reached), n_robots outside 1..8, window odd or outside 4..64, rotate outside
 * {0, 1}, flags != 0, a radius, v_max, w_max, align_tol, goal_tol or dt that is not finite or not positive, both or neither of
 * goals_xy / goals_ab; the robot-count errors of cagym_ig_robot_inputs; CAGYM_E_DEVICE as every launching entry. */
typedef struct cagym_ig_goal_params cagym_ig_goal_params;
int cagym_ig_geodesic(void* env, const cagym_ig_goal_params* params, const uint8_t* mask, const double* goals_xy, const int32_t* goals_ab,
                      float* field, double* goal_xy, uint8_t* active, int32_t* sweeps, void* stream);
int cagym_ig_goal_actions(void* env, const cagym_ig_goal_params* params, const float* field, const double* goal_xy,
                          const uint8_t* active, float* actions, uint8_t* choice, void* stream);
int cagym_ig_goal_status(void* env, const cagym_ig_goal_params* params, const uint8_t* restart_mask, const float* field,
                         const double* goal_xy, uint8_t* active, float* goal_distance, uint8_t* goal_reached, void* stream);

/* ---- View gains and goal proposals: what a place is worth to an IG robot, and the best k places per robot ---------------------------
 * Two launches on `stream`, on demand (no step runs them), no host synchronisation, no global atomics, barriers only.  params of both:
 * cagym_ig_view_params, defined in include/cagym_ig_viewpoints.h (n_points = P, n_robots = R 1..8, k 1..16, flags = 0, radius, range,
 * min_sep, d0); every call validates the whole block.  Cells are those of the belief: i = floor((x + 15) / 0.5), j likewise of y,
 * centre c(i) = i * 0.5 - 15 + 0.25.
 *
 * cagym_ig_view_gain: the mutual information a robot standing at a point would cover turning on the spot (no field of view, no
 * heading), through the walls of the world's CURRENT scenario slot.  points_xy DEVICE [N,P,2] f64 in world metres, or NULL: the 3600
 * cell centres, P = 3600, point j * 60 + i = (c(i), c(j)) - the outputs are then maps [N,60,60] indexed [j, i], and their values are
 * those of a points call on the same points bit for bit.  world_mask DEVICE [N] u8 or NULL (= every world): a world whose byte is 0
 * is skipped, nothing of it is read or written.  Outputs, DEVICE [N,P]: valid u8, n_visible i32, gain f64.
 *   valid <=> x and y are finite, the point's cell lies in 0..59 on both axes, and EDF(x, y) > radius + 0.1 (the planners' feasibility
 *     test, edfMap.get_edf_value_from_pose).  An invalid point has gain = 0 and n_visible = 0.
 *   candidates: cells i in max(0, cell(x - range)) .. min(59, cell(x + range)), j likewise; in range <=> dx dx + dy dy < range range
 *     with dx = c(i) - x (fp64, separate operations); visible <=> edfMap.checkVisibility(point, centre), the sphere trace of
 *     cagym_ig_visible_cells (the own cell at distance 0 is visible).
 *   n_visible = the visible in-range candidates, gain = the sum of the MI cache's values (cell_mi(belief), as cagym_ig_mi_reward reads
 *     them) over them: per lane in candidate order (row-major, lane = candidate mod 64), the 64 lanes in a fixed tree - the same bits
 *     on every call.
 *
 * cagym_ig_propose_goals: one workgroup per (world, robot); mask DEVICE [N,R] u8 or NULL (= every robot): a robot whose byte is 0 is
 * skipped, nothing of it is read or written.  gain_map DEVICE [N,60,60] f64 and valid_map DEVICE [N,60,60] u8: a world's view-gain
 * map; field DEVICE [N,R,60,60] f32: cagym_ig_geodesic's with the robot's own place as the source.
 *   eligible <=> valid != 0, gain > 0 and field finite; utility = gain / ((double)field + d0), one fp64 addition, one fp64 division.
 *   up to k rounds: the eligible, unsuppressed cell of largest utility (of equal ones the smallest j * 60 + i) is chosen, then every
 *   cell with (double)(di di + dj dj) * 0.25 < min_sep min_sep is suppressed, the chosen one included; stop when none is left.
 * Outputs, DEVICE: cells [N,R,k,2] i32 (i, j); xy [N,R,k,2] f64 the centres; utility, gain [N,R,k] f64; distance [N,R,k] f32 the field
 * there; n_found [N,R] i32.  Rows past n_found hold cells = -1, xy = NaN, utility = gain = 0, distance = +inf.
 *
 * Errors, both, before anything is touched: CAGYM_E_STATE before cagym_ig_init; CAGYM_E_INVALID for a NULL params or output (or
 * gain_map, valid_map, field), n_points < 0, n_robots outside 1..8, k outside 1..16, flags != 0, a radius, range, min_sep or d0 that
 * is not finite or not positive; CAGYM_E_DEVICE as every launching entry. */
typedef struct cagym_ig_view_params cagym_ig_view_params;
int cagym_ig_view_gain(void* env, const cagym_ig_view_params* params, const uint8_t* world_mask, const double* points_xy, double* gain,
                       int32_t* n_visible, uint8_t* valid, void* stream);
int cagym_ig_propose_goals(void* env, const cagym_ig_view_params* params, const uint8_t* mask, const double* gain_map,
                           const uint8_t* valid_map, const float* field, int32_t* cells, double* xy, double* utility, double* gain,
                           float* distance, int32_t* n_found, void* stream);

/* ---- Heading-resolved view gains, goal headings and facing: what a POSE is worth, and a goal that says which way to look -----------
 * On `stream`, on demand or opt-in, no host synchronisation, no global atomics, barriers only.
 *
 * cagym_ig_view_gain_headings: cagym_ig_view_gain for a sensor cone.  params: cagym_ig_heading_params, defined in
 * include/cagym_ig_headings.h (n_points = P, n_headings = H 1..16, flags = 0, radius, range, fov, headings[16] in radians).
 * points_xy DEVICE [N,P,2] f64 or NULL (the 3600 cell centres, outputs then [N,60,60,..] indexed [j, i], values those of a points
 * call bit for bit) and world_mask DEVICE [N] u8 or NULL as cagym_ig_view_gain takes them.  Outputs, DEVICE: gain_h [N,P,H] f64 and
 * n_visible_h [N,P,H] i32, either may be NULL; best_heading [N,P] i32, best_gain [N,P] f64, valid [N,P] u8.
 *   valid: cagym_ig_view_gain's rule (finite, inside the map, EDF(x, y) > radius + 0.1).
 *   For a valid point and heading h the counted cells are exactly the mask cagym_ig_visible_cells returns for the pose
 *     (x, y, headings[h]) on the world's current scenario slot with this fov and range: the box with its exclusive upper bound, the
 *     rotation, the cone test `rn < range and |atan2(r1, r0)| < fov / 2` and the sphere trace are the same device functions.
 *   n_visible_h = their number, gain_h = the sum of the MI cache's values over them: per lane in candidate order (row-major over
 *     cell(p - range) .. cell(p + range), lane = candidate mod 64), the 64 lanes in a fixed tree - the same bits on every call.
 *   best_heading = the first index of the largest gain_h, best_gain = that value bit for bit.
 *   An invalid point: best_heading -1, best_gain 0, gain_h and n_visible_h rows 0.
 * Errors, before anything is touched: CAGYM_E_STATE before cagym_ig_init; CAGYM_E_INVALID for a NULL params, best_heading, best_gain
 * or valid, n_points < 0, n_headings outside 1..16, flags != 0, a radius, range or fov that is not finite or not positive, a heading
 * among the first n_headings that is not finite, more than 2^31 - 1 workgroups; CAGYM_E_DEVICE as every launching entry.
 *
 * cagym_ig_goal_face_actions: directly behind cagym_ig_goal_actions, with its params, goal_xy, active and actions; goal_heading
 * DEVICE [N,R] f64 radians, NaN = none.  A robot with an active goal, a finite goal heading and sqrt(dx dx + dy dy) <= goal_tol -
 * the predicate on which cagym_ig_goal_actions stops it - gets the row (0, clip(wrap(goal_heading - heading) / dt, -w_max, w_max)),
 * wrap(a) = (a + pi) mod 2 pi - pi, computed in fp64 and stored as f32; every other row keeps its bytes.
 *
 * cagym_ig_goal_face_status: directly behind cagym_ig_goal_status, on the `active` it left.  goal_facing DEVICE [N,R] u8 = 1 when the
 * robot is active, within goal_tol of its goal point, and either has no finite goal heading or |wrap(goal_heading - heading)| <=
 * face_tol (radians, by value; finite, > 0, else CAGYM_E_INVALID).
 * Errors of the two: as cagym_ig_goal_actions / cagym_ig_goal_status. */
typedef struct cagym_ig_heading_params cagym_ig_heading_params;
int cagym_ig_view_gain_headings(void* env, const cagym_ig_heading_params* params, const uint8_t* world_mask, const double* points_xy,
                                double* gain_h, int32_t* n_visible_h, int32_t* best_heading, double* best_gain, uint8_t* valid,
                                void* stream);
int cagym_ig_goal_face_actions(void* env, const cagym_ig_goal_params* params, const double* goal_xy, const uint8_t* active,
                               const double* goal_heading, float* actions, void* stream);
int cagym_ig_goal_face_status(void* env, const cagym_ig_goal_params* params, double face_tol, const double* goal_xy,
                              const uint8_t* active, const double* goal_heading, uint8_t* goal_facing, void* stream);

/* ---- Team goal assignment: marginal view gains -------------------------------------------------------------------------------------
 * cagym_ig_assign_goals: ONE launch on `stream`, on demand (no step runs it), one workgroup per world, no host synchronisation, no
 * global atomics; two launches give the same bytes.  The sequential-greedy allocation of coverage over the robots' candidate goals:
 * every candidate's visible cell set is a 60 x u64 mask, the team claims masks one robot at a time, and every candidate still open is
 * priced by the mutual information of the cells nobody has claimed yet.  params: cagym_ig_assign_params, defined in
 * include/cagym_ig_assign.h (n_robots = R 1..8, k 1..16, mode, flags = 0, radius, range, d0, fov).
 * Inputs, DEVICE: mask [N,R] u8 or NULL (= every robot) the robots that choose now; cand_xy [N,R,k,2] f64; cand_heading [N,R,k] f64
 * or NULL, an entry that is not finite (NaN) = omnidirectional; cand_distance [N,R,k] f32; claim [N,R] u8 or NULL, with it claim_xy
 * [N,R,2] f64 and claim_heading [N,R] f64 or NULL.
 *   cell set of a pose: with a finite heading exactly the mask cagym_ig_visible_cells returns for (x, y, heading) with this fov and
 *     range; without one exactly the cells cagym_ig_view_gain counts at the point with this range.  A point that fails
 *     cagym_ig_view_gain's `valid` rule at this radius has the empty set.
 *   claimed starts as the union of the cell sets of (claim_xy, claim_heading) of every robot with claim != 0 and mask == 0; a masked
 *     robot's claim byte is ignored.
 *   marginal gain of a candidate = the double cagym_ig_mi_reward returns for cells & ~claimed, bit for bit.
 *   eligible <=> the point is valid, cand_distance is finite and the marginal gain is > 0; utility = marginal / ((double)distance + d0).
 *   mode CAGYM_IG_ASSIGN_SLOT: the masked robots take turns in slot order, each taking its eligible candidate of largest utility (of
 *     equal ones the smaller index), then claimed |= cells; none eligible: choice -1, nothing claimed.
 *   mode CAGYM_IG_ASSIGN_BEST: up to R rounds, each assigning the eligible (robot, candidate) of largest utility among the masked
 *     robots still open (ties: the smaller slot, then the smaller index); the rounds stop when nothing is eligible.
 * Outputs, DEVICE: choice [N,R] i32 the candidate or -1; order [N,R] i32 the round (0-based; SLOT: the robot's turn) in which it was
 * assigned or -1; marginal, utility [N,R] f64 the chosen candidate's at that round, 0 when unassigned; claimed [N,60] u64 the final
 * union, seeds included; masks [N,R,k,60] u64 every candidate's cell set before any claim (required: the kernel's workspace);
 * round_gain [N,R,R,k] f64 or NULL, indexed [round, robot, candidate]: the marginal gain of every candidate priced in that round
 * (SLOT: the robot whose turn it is; BEST: every robot still open), NaN for everything else - robots assigned or outside the mask,
 * invalid points, non-finite distances, rounds that were not played.  Rows of robots outside the mask keep every byte (masks
 * included); a world without a masked robot is neither read nor written, claimed included.
 * Errors, before anything is touched: CAGYM_E_STATE before cagym_ig_init; CAGYM_E_INVALID for a NULL params, cand_xy, cand_distance
 * or required output, n_robots outside 1..8, k outside 1..16, a mode outside {0, 1}, flags != 0, a radius, range, d0 or fov that is
 * not finite or not positive, claim without claim_xy; CAGYM_E_DEVICE as every launching entry. */
typedef struct cagym_ig_assign_params cagym_ig_assign_params;
int cagym_ig_assign_goals(void* env, const cagym_ig_assign_params* params, const uint8_t* mask, const double* cand_xy,
                          const double* cand_heading, const float* cand_distance, const uint8_t* claim, const double* claim_xy,
                          const double* claim_heading, int32_t* choice, int32_t* order, double* marginal, double* utility,
                          uint64_t* claimed, uint64_t* masks, double* round_gain, void* stream);

/* ---- Route gains: what a robot sees on the way to a candidate goal ------------------------------------------------------------------
 * cagym_ig_route_gains: ONE launch on `stream`, on demand (no step runs it), one workgroup of 256 threads per world, no host
 * synchronisation, no global atomics, no unbounded loop; two launches give the same bytes.  Every candidate cell's shortest path is
 * walked back on the robot's own geodesic field, the sensor cone is taken at way-points along it, and the union is priced.  params:
 * cagym_ig_route_params, defined in include/cagym_ig_route.h (n_robots = R 1..8, k 1..16, stride >= 1, flags = 0, radius, range,
 * fov, d0).
 * Inputs, DEVICE: mask [N,R] u8 or NULL (= every robot); field [N,R,60,60] f32, each robot's geodesic field with its own position
 * as the source, as cagym_ig_geodesic writes it; cand_cells [N,R,k,2] i32 (i, j), a row with a cell outside 0..59 has no route;
 * cand_heading [N,R,k] f64 or NULL; exclude [N,60] u64 or NULL, cells already spoken for (e.g. cagym_ig_assign_goals' claimed).
 *   walk: from the candidate's cell q_0 (field finite, else no route) to the neighbour cagym_ig_goal_actions would drive to - E, N,
 *     W, S, NE, NW, SW, SE in this order, key fl32(field[n] + cost) over finite values only, a diagonal only with both orthogonal
 *     neighbours finite, the first of equal smallest keys - until the cell whose field is 0, q_n.  A cell without such a neighbour,
 *     a move that does not lower the field value, or more than 3600 moves: no route.
 *   travel order: p_t = q_{n-t}; the heading into p_t is that of the move p_{t-1} -> p_t, the double m * (M_PI / 4) with m = 0, 2, 4,
 *     -2, 1, 3, -3, -1 for E .. SE.
 *   way-points: t = stride, 2 stride, .. with t < n and t <= 16 stride; truncated = 1 when a t < n beyond 16 stride was dropped.
 *     A way-point's cell set is exactly the mask cagym_ig_visible_cells returns for (centre of its cell, heading into it) with this
 *     fov and range.
 *   route = the union of the way-point sets; terminal = the candidate's own set at its cell's centre by cagym_ig_assign_goals' rule
 *     (finite cand_heading: the cone; none: a robot turning on the spot; EDF(centre) <= radius + 0.1: empty); total = route | terminal.
 *   route_gain / total_gain = the double cagym_ig_mi_reward returns for route & ~exclude / total & ~exclude, bit for bit;
 *     utility = total_gain / ((double)field[q_0] + d0).
 *   best = the candidate with a route and total_gain > 0 of largest utility, of equal utilities the smaller index; none: -1.
 * Outputs, DEVICE: route_masks, total_masks [N,R,k,60] u64; route_gain, total_gain, utility [N,R,k] f64 (no route: 0, empty masks);
 * n_path [N,R,k] i32 the moves n, -1 = no route; n_way [N,R,k] i32; truncated [N,R,k] u8; best [N,R] i32; way_cells [N,R,k,16,2]
 * i32 or NULL and way_dir [N,R,k,16] i8 or NULL: the way-points in travel order as (i, j) and the direction of the move into them
 * (0..7 in the order above), rows past n_way -1.  Rows of robots outside the mask keep every byte; a world without a masked robot
 * is neither read nor written.
 * Errors, before anything is touched: CAGYM_E_STATE before cagym_ig_init; CAGYM_E_INVALID for a NULL params, field, cand_cells or
 * required output, n_robots outside 1..8, k outside 1..16, stride < 1, flags != 0, a radius, range, fov or d0 that is not finite or
 * not positive; CAGYM_E_DEVICE as every launching entry. */
typedef struct cagym_ig_route_params cagym_ig_route_params;
int cagym_ig_route_gains(void* env, const cagym_ig_route_params* params, const uint8_t* mask, const float* field,
                         const int32_t* cand_cells, const double* cand_heading, const uint64_t* exclude, uint64_t* route_masks,
                         uint64_t* total_masks, double* route_gain, double* total_gain, double* utility, int32_t* n_path,
                         int32_t* n_way, uint8_t* truncated, int32_t* best, int32_t* way_cells, int8_t* way_dir, void* stream);

/* ---- Per-robot credit for the team reward: own, exclusive and difference rewards ----------------------------------------------------
 * cagym_ig_observe gives a team ONE number per world; this call says whose cone earned it.  ONE launch on `stream` (one workgroup of
 * 256 threads per world), to be enqueued directly behind cagym_ig_observe (and behind cagym_ig_context_window where there is one) with
 * the same obs_oas, restart_mask and flags; no host synchronisation, no global atomics, barriers only; two launches give the same
 * bytes; it writes nothing of the handle.  params: cagym_ig_credit_params, defined in include/cagym_ig_credit.h (n_robots = R 1..8,
 * flags, detect_range fp32, fov_rad, range).  belief and mi below are the world's belief and MI cache as the observe launch left them.
 * For world w (skipped - nothing read or written - with CAGYM_IG_OBSERVE_ONLY_RESTARTED when it is not restarted) and its robots
 * r = 0..R-1, the active CAGYM_POL_IGMCTS slots in slot order (a row past the world's team: no pose, no detections, V_r empty):
 *   pose and detections of robot r as cagym_ig_robot_inputs computes them;
 *   V_r = the mask cagym_ig_visible_cells returns for (pose, fov_rad, range) on the world's current scenario slot; U = the union of
 *     all V_r; U_-r = the union of V_s over s != r;
 *   f_r(q) = 1.5 when cell q passes cagym_ig_update_belief's detection test for robot r (a detection within sqrt(0.5) 0.5 + 0.01 of
 *     the cell's centre, both rotated into the robot's frame), else 0.66;
 *   gain = the MI sum over U - cagym_ig_observe's gain[w], bit for bit;
 *   own[r] = the MI sum over V_r, exclusive[r] = the MI sum over V_r & ~U_-r - both bit for bit what cagym_ig_mi_reward returns for
 *     that mask;
 *   loo[r] = the sum over q in U_-r of (q in V_r ? cell_mi(belief[q] / f_r(q)) : mi[q]), in cagym_ig_mi_reward's order (thread
 *     q % 256 accumulates its cells strided, then the halving tree); an empty U_-r sums to +0.0: what the gain would have been had
 *     robot r not looked;
 *   difference[r] = gain - loo[r], the difference reward.  A row past the team: own = exclusive = difference = 0, loo = gain.
 * Outputs, DEVICE, caller-owned, each may be NULL: gain [N] f64; robot_observed [N,R,60] u64 = V_r; credit [N,R,3] f64 = (own,
 * exclusive, difference), raw as gain is; loo [N,R] f64; reward [N,R,3] f64 = credit, but 0 for a world restarted in this launch, as
 * team_reward is; the accumulators running, sum, last [N,R,3] f64 and episodes [N] i32, by cagym_ig_observe's statements per robot
 * and kind: if restarted: with CAGYM_IG_EPISODE_FOLD sum += running, last = running, episodes[w] += 1; running = 0; then
 * running += credit.  running NULL: no accumulator but episodes is touched.
 * Errors: CAGYM_E_INVALID for a NULL env, params or obs_oas, n_robots outside 1..8, unknown flags, a non-finite or non-positive
 * fov_rad, range or detect_range; CAGYM_E_STATE before cagym_ig_init; CAGYM_E_DEVICE as every launching entry.  A refused call
 * writes nothing. */
typedef struct cagym_ig_credit_params cagym_ig_credit_params;
int cagym_ig_credit(void* env, const cagym_ig_credit_params* params, const float* obs_oas, const uint8_t* restart_mask, double* gain,
                    uint64_t* robot_observed, double* credit, double* loo, double* reward, double* running, double* sum, double* last,
                    int32_t* episodes, void* stream);

/* ---- Per-scenario episode records under auto-reset (experiments/src/env_utils.py:41-62 reads them from prev_episode_agents;
 * process_full_test_suite_pickles.py:90-116 turns them into the published table) ---------------------------------------------------
 * An auto-resetting step re-initialises a finished world inside the launch that finished it; the recorder rebuilds what the reference
 * reads at the end of an episode from the step's OUTPUTS (flags, reward, game_over) and the scenario pool, in a launch of its own
 * beside the step kernels (csrc/cagym_episode_records.h).  Agent.t follows from the flags alone: 0 at the start of an episode, += dt
 * every step unless the agent's AT_GOAL bit was set in the flags of the previous step of the same episode (agent.py:147-159, 184-186).
 * Table, one row per scenario s of the pool, written when an episode on s ends:
 *   t [S,M] f64, extra_t [S,M] f64 = t - (|start - goal| - 0.75) / pref_speed (agent.py:59), flags [S,M] u8 the terminal CAGYM_FLAG_*
 *   byte, ret [S] f64 = sum of agent 0's reward in step order (score += rew[0]), steps [S] i32, outcome [S] i32 (bit 0: any agent
 *   IN_COLLISION, bit 1: all agents AT_GOAL, bit 2: any agent neither; env_utils.py:55-60), count [S] i32 finished episodes seen.
 *   Slots >= the pool's n_agents[s] hold zeros and take no part in outcome.
 * Running, per world: t_run [N,M] f64, ret_run [N] f64, steps_run [N] i32, atgoal_run [N] u32 (bit per slot), cursor [N] i32 = the
 * episode index the recorder believes the world is on (row s = (w + cursor * N) % S).  desync: one i32 word.
 * keep: CAGYM_EPREC_KEEP_FIRST: a row is written by the first episode that ends on it and later episodes only count (a suite's
 *   table is complete and stable once every count >= 1); CAGYM_EPREC_KEEP_LAST: the newest finished episode overwrites the row.
 *   When two worlds end episodes on one scenario, the order is (step, world): one of them owns the whole row, count adds both.
 * cagym_episode_records_init: allocate (once) and clear; a second call clears again and may change keep.
 * cagym_episode_records_update: ONE launch over T consecutive steps: flags [T,N,M] u8, reward [T,N,M] f32, game_over [T,N] u8 (DEVICE).
 *   CONTRACT: the outputs of auto-reset stepping only (cagym_step_autoreset, cagym_step_finish with auto_reset, cagym_rollout with
 *   auto_reset), every step exactly once and in order, enqueued behind the step(s) that wrote them and before the next stepping call
 *   on the handle.  No argument advances on the host, so the call can be captured in a graph with the steps.  After the last slice
 *   the kernel compares cursor and steps_run of every world with the episode index and episode length the step kernels keep; on a
 *   mismatch (a skipped, doubled or non-auto-reset step) it adds 1 to desync, takes the handle's values and drops the world's
 *   running values.  A pool whose n_scenarios is a multiple of n_worlds has one writer per row and runs on the whole device; any
 *   other pool is walked by one workgroup in step order (rows may be shared).
 * cagym_episode_records_restart: the masked worlds (DEVICE [N] u8, NULL = all) forget the episode in progress and take the handle's
 *   episode index; clear_table != 0 also clears the table and desync.
 * cagym_episode_records_get: zero-copy DEVICE views, owned by the handle.
 * Once initialised: a successful cagym_reset enqueues the restart for its mask on its stream (an abandoned episode leaves no record);
 * a successful cagym_set_scenarios / cagym_generate_scenarios / cagym_generate_reference_scenarios clears the table and every running
 * value (the table describes the pool).  Handles that never called init behave as before.
 * Errors: CAGYM_E_INVALID for a NULL env; CAGYM_E_STATE before cagym_set_scenarios, and for update / restart / get before init;
 * CAGYM_E_INVALID for a NULL flags / reward / game_over / out, T < 1 or an unknown keep; CAGYM_E_DEVICE as every launching entry. */
enum { CAGYM_EPREC_KEEP_FIRST = 0, CAGYM_EPREC_KEEP_LAST = 1 };
typedef struct cagym_episode_record_ptrs {
    const double *t, *extra_t;
    const uint8_t* flags;
    const double* ret;
    const int32_t *steps, *outcome, *count;
    const double *t_run, *ret_run;
    const int32_t* steps_run;
    const uint32_t* atgoal_run;
    const int32_t* cursor;
    const int32_t* desync;
} cagym_episode_record_ptrs;
int cagym_episode_records_init(void* env, int keep, void* stream);
int cagym_episode_records_update(void* env, const uint8_t* flags, const float* reward, const uint8_t* game_over, int T, void* stream);
int cagym_episode_records_restart(void* env, const uint8_t* world_mask, int clear_table, void* stream);
int cagym_episode_records_get(void* env, cagym_episode_record_ptrs* out);

/* ---- Append-only episode log under auto-reset, streamed pools included (csrc/cagym_episode_log.h) -----------------------------------
 * The records table above has one row per pool slot, which a streamed pool reuses (cagym_stream_*): a streaming handle refuses it.
 * The log is not keyed by slot: a device ring of `capacity` rows, ONE ROW PER FINISHED EPISODE, rebuilt from the same step outputs by
 * launches of its own behind the auto-resetting step(s).  No step, reset, roll-out or refill kernel knows of it.
 * Row columns (structure of arrays, L = capacity rows):
 *   key [L] u32 = (uint32_t)(w + e * N), the stream key of the episode that ended (world w, episode index e; while
 *   cagym_stream_replay_* is armed: the key its slot was really generated from); world, episode [L] i32;
 *   slice [L] i64, the index of the slice that ended the episode counted over all update calls since init / clear;
 *   steps [L] i32; ret [L] f64 (sum of agent 0's reward in step order); outcome [L] i32 (the records' bits: 1 any collision, 2 all at
 *   goal, 4 any neither); n_agents, n_obst [L] i32 from the pool row of the episode's slot (w + e * N) % S (n_obst 0 without
 *   rectangles); t, extra_t [L,M] f64 and flags [L,M] u8 as the records define them, zeros at slots >= n_agents.
 *   t, extra_t, ret, steps, outcome and the masking are computed by the recorder's own device functions: log and table hold the same
 *   doubles.  With constant stream parameters the scenario of (w, e) is a pure function of (params, w, e) (see cagym_stream_*), so a
 *   logged episode is reproducible: generate a plain pool of more than `key` slots with the same arguments and read row `key`.
 * Running, per world and the log's own (records and log may both be initialised on a fixed pool; they share no state): t_run [N,M]
 *   f64, ret_run [N] f64, steps_run [N] i32, atgoal_run [N] u32, cursor [N] i32; desync, one i32 word with the recorder's meaning;
 *   head, one u64 word: the number of rows ever appended since init / clear.
 * ORDER (deterministic): the rows of one update are appended world-major - ascending world, inside a world ascending slice -;
 *   updates append in call order; row number i (0-based, i < head) lives at ring index i % capacity.  An update that finishes
 *   n > capacity episodes writes only its last `capacity` rows in that order, the others are skipped; head still grows by n.
 *   Valid rows: the min(head, capacity) newest, oldest first from ring index head % capacity when head > capacity, else from 0.
 * cagym_episode_log_init: allocate (the running values once, the ring once per capacity) and clear; a second call clears again and
 *   may change the capacity (that synchronises the device and frees the old ring).
 * cagym_episode_log_update: at most three launches (count per world, one exclusive scan over the N counts, write), chained by stream
 *   order only.  Inputs and CONTRACT as cagym_episode_records_update: the outputs of auto-reset stepping only, every step exactly once
 *   and in order, behind the step(s) that wrote them and before the next stepping call.  WHILE STREAMING ALSO BEFORE
 *   cagym_stream_refill: the update reads the pool row of the slot of the episode that ended, and the next refill regenerates that
 *   slot (it is the slot of episode e + n_scenarios / n_worlds).  For a world that lapped its ring inside a roll-out the row describes
 *   the scenario that actually ran - the slot's content - while its key is still w + e * N; cagym_stream_get's n_lapped tells a caller
 *   that this happened.  No argument advances on the host: the call can be captured in a graph with the steps.  desync as the
 *   recorder's: after the last slice cursor / steps_run are compared with the handle's episode index and length.
 * cagym_episode_log_restart: the masked worlds (DEVICE [N] u8, NULL = all) forget the episode in progress and take the handle's
 *   episode index; clear_rows != 0 also zeroes every row, head, the slice counter and desync.
 * cagym_episode_log_get: zero-copy DEVICE views, owned by the handle (the ring's views change when init changes the capacity).
 * Once initialised: a successful cagym_reset enqueues the restart for its mask (an abandoned episode leaves no row); a successful
 * cagym_set_scenarios / cagym_generate_scenarios / cagym_generate_reference_scenarios / cagym_stream_scenarios clears the running
 * values and takes the handle's episode indices - the rows, head, the slice counter and desync stay: a log is history and every row is
 * self-contained.  cagym_stream_scenarios and cagym_stream_set_params do not refuse a handle with a log.  cagym_restore and cagym_fork
 * return CAGYM_E_STATE while a log is initialised (its running rows would describe another timeline, as the records' would);
 * cagym_snapshot stays allowed.  Handles that never called init behave as before.
 * Errors: CAGYM_E_INVALID for a NULL env; CAGYM_E_STATE before a pool is installed, and for update / restart / get before init;
 * CAGYM_E_INVALID for a NULL flags / reward / game_over / out, T < 1 or capacity < 1; CAGYM_E_DEVICE as every launching entry. */
struct cagym_episode_log_ptrs {
    const uint32_t* key;
    const int32_t *world, *episode;
    const int64_t* slice;
    const int32_t* steps;
    const double* ret;
    const int32_t *outcome, *n_agents, *n_obst;
    const double *t, *extra_t;
    const uint8_t* flags;
    const double *t_run, *ret_run;
    const int32_t* steps_run;
    const uint32_t* atgoal_run;
    const int32_t* cursor;
    const uint64_t* head;
    const int32_t* desync;
    int32_t capacity;
};
typedef struct cagym_episode_log_ptrs cagym_episode_log_ptrs;
int cagym_episode_log_init(void* env, int capacity, void* stream);
int cagym_episode_log_update(void* env, const uint8_t* flags, const float* reward, const uint8_t* game_over, int T, void* stream);
int cagym_episode_log_restart(void* env, const uint8_t* world_mask, int clear_rows, void* stream);
int cagym_episode_log_get(void* env, cagym_episode_log_ptrs* out);

/* ---- Episode log of the information-gathering team: belief and target-search metrics (csrc/cagym_ig_episode_log.h) ---------------
 * The log above rebuilds its rows from the step's outputs.  What a target search is judged by lives in the belief, and the chain puts
 * a finished world's belief back to the prior in the launch that folds its return (cagym_ig_observe, cagym_ig_episode_boundary).
 * This log goes BETWEEN the auto-resetting step and that launch: ONE ROW PER FINISHED TEAM EPISODE in a device ring of `capacity`
 * rows.  No existing kernel knows of it; a handle that never called init runs none of its code.
 * Row columns (structure of arrays, L = capacity rows):
 *   key [L] u32 = (uint32_t)(w + e * N), the stream key of the episode that ended; world, episode [L] i32; slice [L] i64, the index
 *   of the update call that appended the row, counted since init / clear; steps [L] i32, the env steps of the episode;
 *   ret [L] f64, the team return: running[w] of cagym_ig_get_episode_stats, plus team_reward[w] when the update is given a
 *     team-reward pointer - the one fp64 add cagym_ig_episode_boundary makes before it folds, so ret equals, bit for bit, the
 *     `last` the boundary / observe launch behind the update leaves;
 *   n_targets, n_found [L] i32 and found_at [L,M] i32 per agent slot: -2 the slot is no target, -1 a target never found, else the
 *     1-based step of the episode at which the log first saw it found (below);
 *   entropy [L] f64 = the sum over the 3600 belief cells of -(P ln P + (1 - P) ln(1 - P)), P = r / (r + 1), r the cell's odds, in
 *     nats (a side whose P or 1 - P has reached 0 in fp64 contributes its limit, 0); residual_mi [L] f64 = the sum of the cells'
 *     cached mutual information (what is left to gain); n_touched [L] i32 = the cells whose odds differ from the prior 1.0.
 *     The three sums run in a fixed order: equal from run to run and between two handles that hold the same belief.
 * Running, per world: steps_run [N] i32, found_run [N,M] i32 (-1 or the step), cursor [N] i32; head, one u64 word: rows ever
 *   appended since init / clear; desync, one i32 word.
 * TARGETS: the STATIC agents of the episode's pool slot s = (w + e * N) % S - slot i with policy[s][i] == CAGYM_POL_STATIC and
 *   i < n_agents[s], at (agents6[s][i][0], agents6[s][i][1]); they are what cagym_ig_robot_inputs reports as detections.  Target i
 *   is FOUND at the first update at which belief[w][j][i'] >= odds_found for the cell i' = floor((x + 15) / 0.5), j likewise of y
 *   (the indexing of cagym_ig_update_belief); a target outside the map is never found.  found_run = steps_run then: exactly that
 *   many belief updates of the episode have been applied, whether a planner updates before its move or a learner's
 *   cagym_ig_observe behind the previous step (or behind the reset).
 * ORDER as the log's above: the rows of one update are appended in ascending world order, updates in call order, row number i lives
 *   at ring index i % capacity; an update that finishes more than `capacity` episodes writes its last `capacity` rows.
 * cagym_ig_episode_log_init: allocate (the running values once, the ring once per capacity) and clear; a second call clears again
 *   and may change capacity (that synchronises the device and frees the old ring) and odds_found = p / (1 - p), divided by the caller.
 * cagym_ig_episode_log_update: two launches chained by stream order (one workgroup that decides every world's row number by an
 *   exclusive count of the finished worlds before it and is the single writer of head and desync; one workgroup per world), no
 *   atomics, no host synchronisation.  CONTRACT: once per cagym_step_autoreset, behind it, with the game_over [N] it wrote, and
 *   BEFORE the cagym_ig_observe / cagym_ig_episode_boundary of that step and before cagym_stream_refill (which regenerates the slot of
 *   the episode that ended).  team_reward [N] f64 DEVICE or NULL: the pointer that boundary launch gets.  For a finished world
 *   (game_over[w] != 0) the handle's episode index must have advanced by one past the log's cursor, for any other world it must
 *   equal it; a world where it does not - a skipped or doubled update, a step without auto-reset - counts into desync, logs
 *   nothing in that call and takes the handle's episode index.  A world that lapped its ring inside a roll-out logs the scenario
 *   that really ran under the key it should have met (cagym_stream_get's n_lapped tells).
 * cagym_ig_episode_log_restart: the masked worlds (DEVICE [N] u8, NULL = all) forget the episode in progress and take the handle's
 *   episode index; clear_rows != 0 also zeroes every row, head, the call counter and desync.  A successful cagym_reset enqueues it
 *   for its mask, a new pool for every world (rows kept), as for the log above.
 * cagym_ig_episode_log_get: zero-copy DEVICE views (cagym_ig_episode_log_ptrs, defined in include/cagym_ig_episode_log.h).
 * The log is in no snapshot and no checkpoint.  While it is initialised cagym_restore and cagym_fork return CAGYM_E_STATE (its
 * running values would describe another timeline): cagym_restore behind every other refusal it makes, cagym_fork behind every other
 * but its CAGYM_E_UNSUPPORTED after cagym_ig_init, which every handle that holds this log would meet.
 * Errors: CAGYM_E_INVALID for a NULL env; CAGYM_E_STATE before cagym_ig_init, and for update / restart / get before init;
 * CAGYM_E_INVALID for capacity < 1, a non-finite or non-positive odds_found, a NULL game_over or out; CAGYM_E_DEVICE as every
 * launching entry. */
typedef struct cagym_ig_episode_log_ptrs cagym_ig_episode_log_ptrs;
int cagym_ig_episode_log_init(void* env, int capacity, double odds_found, void* stream);
int cagym_ig_episode_log_update(void* env, const uint8_t* game_over, const double* team_reward, void* stream);
int cagym_ig_episode_log_restart(void* env, const uint8_t* world_mask, int clear_rows, void* stream);
int cagym_ig_episode_log_get(void* env, cagym_ig_episode_log_ptrs* out);

/* ---- Per-world state snapshot, restore and fork (csrc/cagym_snapshot.h) -------------------------------------------------------------
 * The env can be put back where it was (checkpoint / resume, rewind) and a world can continue as a copy of another one (look-ahead:
 * "try these K actions from this state").  One copy kernel beside the step kernels; no step, reset or roll-out kernel knows of it.
 * A blob is [n, row_bytes] caller-owned DEVICE bytes, 16-byte aligned.  A row holds everything the handle keeps per world except
 * the split step's hand-over: a 16-byte header {origin world id, CAGYM_SNAP_MAGIC, 0, 0}, then (CAGYM_SNAP_CORE) the 18 fp64
 * per-agent arrays (the cagym_state_ptrs ones and coop), action, status, step_num, n_observed, and per world n_agents, episode,
 * the running episode length and return, stat_return, stat_episodes, stat_steps, stat_outcomes; after cagym_ig_init also
 * (CAGYM_SNAP_IG) the world's belief grid, its MI cache and the four cagym_ig_get_episode_stats accumulators.  Every field starts at
 * a multiple of 16 inside the row and row_bytes is a multiple of 16.  The scenario pool is NOT part of a blob: a world's scenario is
 * computed, (world + episode * N) % S, so putting `episode` back puts the scenario back - into the pool the handle holds THEN
 * (resume in a fresh handle: install the same pool first).  The caller's output buffers are not part of it either.
 * cagym_snapshot_layout_of: the handle's layout (host only, no launch).  It changes when cagym_ig_init runs.
 * cagym_snapshot: row r of the blob <- world worlds[r] (DEVICE [n] i32; NULL: worlds 0..N-1, and n must be N).
 * cagym_restore: blob row rows[r] (DEVICE [n] i32; NULL: rows 0..n-1) -> the origin world its header names; there is no destination
 *   argument.  `layout` is the one the blob was taken with; it must equal the handle's own in every field (same N, M, S,
 *   max_obstacles, IG-ness), which lets a blob restore into a fresh handle of the same shape.
 * cagym_fork: world dst[r] continues as a copy of world src[r] (DEVICE [n] i32 each): every field of a row except dst's own episode
 *   index and stat_* (the running episode length and return ARE copied), and the pool rows of src's current scenario slot over
 *   dst's current slot (start / goal / speed / radius rows, the heading buffer whether or not headings are in use, coop, policy,
 *   dynamics, n_agents, n_obst and, with rectangles, the raster, the rectangles and their prepared form) - so dst steps against
 *   src's rectangles and a later cagym_reset of dst re-initialises it from the forked scenario.  No kernel needs an indirection.
 * All work is enqueued on `stream`; no call allocates or synchronises the host, so all three can be captured in a graph.
 * cagym_restore and cagym_fork void a pending cagym_step_begin; cagym_snapshot does not.
 * Every id read from a list, and the origin id of a blob row, is checked on the device: an id outside [0, N) (or a row without
 * the magic) makes that row's workgroup return without touching memory.
 * PRECONDITIONS the library cannot check without reading device memory: the dst ids of one cagym_fork are distinct and none is
 * also a src of the same call; the rows of one cagym_restore name distinct origin worlds and are smaller than the number of rows the
 * blob holds.  Violating the first three gives an unspecified mix of the candidates, never a fault; a row id in [n of the blob, N)
 * reads past the caller's blob (the library does not know its size; BatchedCollisionAvoidanceEnv.restore masks such ids).
 * Errors, in this order: CAGYM_E_INVALID for a NULL env; CAGYM_E_STATE before cagym_set_scenarios; CAGYM_E_INVALID for n < 0 or
 * n > N, a NULL blob or one that is not 16-byte aligned, NULL worlds with n != N, NULL src / dst with n > 0, a NULL layout or one
 * that differs from the handle's own in any field; CAGYM_E_STATE for restore / fork while episode records are initialised (their
 * running rows would describe another timeline: detach the records first) and, for the same reason, while an episode log
 * (cagym_episode_log_init) is initialised; CAGYM_E_UNSUPPORTED for fork on a handle whose
 * n_scenarios is not a multiple of n_worlds (two worlds can share a slot, the overwrite could hit a third) or after cagym_ig_init
 * (the per-slot distance field is not copied); CAGYM_E_DEVICE as every launching entry. */
#define CAGYM_SNAP_MAGIC 0x43475331u /* "CGS1" */
#define CAGYM_SNAP_VERSION 1
enum { CAGYM_SNAP_CORE = 1, CAGYM_SNAP_IG = 2 };
struct cagym_snapshot_layout {
    uint32_t magic, version;
    int32_t n_worlds, max_agents, n_scenarios, max_obstacles;
    uint32_t fields;    /* CAGYM_SNAP_CORE | CAGYM_SNAP_IG */
    uint32_t reserved;  /* 0 */
    uint64_t row_bytes;
};
typedef struct cagym_snapshot_layout cagym_snapshot_layout;
int cagym_snapshot_layout_of(void* env, cagym_snapshot_layout* out);
int cagym_snapshot(void* env, const int32_t* worlds, int n, void* blob, void* stream);
int cagym_restore(void* env, const cagym_snapshot_layout* layout, const void* blob, const int32_t* rows, int n, void* stream);
int cagym_fork(void* env, const int32_t* src, const int32_t* dst, int n, void* stream);

/* ---- Fresh scenarios streamed into the pool under auto-reset (csrc/cagym_stream.h) ---------------------------------------------------
 * The reference draws a new random world at every reset() (_init_agents, collision_avoidance_env.py:403-442, with the curriculum of
 * :419-438 changing the sampler set as training goes on).  A fixed pool replays its scenarios after S / N episodes; streaming turns
 * the pool into a ring of depth k = S / N per world instead: world w owns slots w, w + N, ..., w + (k - 1) N, and slot
 * (w + e * N) % S holds the scenario of its episode e - the one cagym_generate_reference_scenarios' samplers draw for the stream key
 * v = (uint32_t)(w + e * N), which takes the place of the scenario index in every u(k), the kind-pick stream included.  With constant
 * parameters the scenario of (w, e) is a pure function of (params, w, e): row v of a plain pool of more than v slots generated with
 * the same arguments, bit for bit (agents, policies, dynamics, counts, coop, rectangles, RVO prep rows, raster).  Keys wrap at 2^32:
 * once w + e * N passes 2^32 the stream repeats the scenarios of the keys it started with.
 * No step, reset or roll-out kernel knows of the stream: they keep deriving the slot from episode[w].
 * cagym_stream_scenarios: validates exactly as cagym_generate_reference_scenarios (same codes and messages, the obstacle-capacity check
 *   included) and refuses besides: n_scenarios % n_worlds != 0 or n_scenarios < 2 * n_worlds (CAGYM_E_INVALID); a handle with
 *   information-gain state (cagym_ig_init done) or a parameter set that can place CAGYM_POL_IGMCTS agents (CAGYM_E_UNSUPPORTED: the
 *   per-slot distance field would need a rebuild); initialised episode records (CAGYM_E_STATE: their table is per pool slot).  Fills
 *   all S slots, slot r from key r - the pool is what cagym_generate_reference_scenarios writes - commits the handle state as that call
 *   does, sets next_episode[w] = k and restarts the counters (generated = S, n_failed = the fill's count, also copied to
 *   *n_failed_host when that is not NULL, which synchronises `stream`; n_lapped = 0).  A refused call leaves the handle as it was.
 *   The first call allocates the words of cagym_stream_get.
 * cagym_stream_refill: ONE launch on `stream`, no host synchronisation, no allocation; enqueue it behind every call that can advance
 *   an episode counter (cagym_step_autoreset, cagym_step_finish with auto_reset, cagym_rollout with auto_reset - once behind the
 *   launch -, cagym_reset with advance_episode) and before the next such call.  CAGYM_E_STATE on a handle that is not streaming.
 *   Per world it reads episode[w] and next_episode[w].  next_episode[w] <= episode[w]: the world has lapped - it started an episode on
 *   a slot that was never refilled (more than k - 1 episodes finished between two refills, which only a roll-out can do); it is
 *   counted once in n_lapped and its current slot is left alone.  It generates the episodes max(next_episode, episode + 1) ..
 *   episode + k - 1 into their slots, sets next_episode[w] = episode[w] + k and adds to generated and n_failed.  The slot of a world's
 *   current episode is never written, and S % N == 0 gives every slot one writer.  A world that finished nothing costs two loads.
 *   The parameter set is a by-value kernel argument: a graph that captured the call keeps the set it was captured with.
 * cagym_stream_set_params: the reference's curriculum switch.  Same validation and refusals; takes effect for the slots later refills
 *   generate (the seed may change too); scenarios already in the ring stay, so a world meets the new set k - 1 episodes later.  While
 *   the stream runs, the handle's flags (RVO agents present, RVO agents among rectangles) are the union of what both sets imply; a
 *   change of them voids a pending cagym_step_begin.  CAGYM_E_STATE on a handle that is not streaming.
 * cagym_stream_get: zero-copy DEVICE views, owned by the handle: next_episode [N] i32, generated u64, n_failed i32, n_lapped i32.
 *   CAGYM_E_STATE before the first cagym_stream_scenarios; they stay readable after the stream stopped.
 * cagym_stream_stop: ends the stream (the pool stays as it is); a successful cagym_set_scenarios, cagym_generate_scenarios or
 *   cagym_generate_reference_scenarios does the same.
 * While streaming: cagym_restore and cagym_fork return CAGYM_E_UNSUPPORTED (the ring is not part of a snapshot; cagym_snapshot stays
 * allowed), cagym_ig_init CAGYM_E_UNSUPPORTED (an exploration stream, below, accepts it) and cagym_episode_records_init CAGYM_E_STATE.
 * Not streamed: cagym_generate_scenarios' own parameter struct (the RANDOM_POSITIONS kind covers its rule). */
struct cagym_stream_ptrs {
    const int32_t* next_episode; /* [N] first episode of world w whose slot has not been generated */
    const uint64_t* generated;   /* slots generated since cagym_stream_scenarios, its fill included */
    const int32_t* n_failed;     /* agents and rectangles whose rejection loop hit max_tries, since then */
    const int32_t* n_lapped;     /* times a world started an episode on a slot that had not been refilled */
};
typedef struct cagym_stream_ptrs cagym_stream_ptrs;
int cagym_stream_scenarios(void* env, const cagym_gen2_params* params, int32_t* n_failed_host, void* stream);
int cagym_stream_refill(void* env, void* stream);
int cagym_stream_set_params(void* env, const cagym_gen2_params* params);
int cagym_stream_get(void* env, cagym_stream_ptrs* out);
int cagym_stream_stop(void* env);

/* ---- Replay of failed scenarios from the episode log, inside the stream (csrc/cagym_replay.h) ----------------------------------------
 * On a cagym_stream_scenarios stream, an optional REPLAY BUFFER of stream keys on the device.  A harvest launch fills it from the
 * episode log (the rows whose outcome matches a mask), a caller may push keys directly, and once armed the refill decides for each
 * slot it generates, by a counter-based draw, between the fresh key w + e * N and a key sampled from the buffer - with replacement:
 * nothing is consumed, no workgroup waits on another, atomics on counters only, everything stream-ordered, no host synchronisation
 * and no allocation after init.  No step, reset or roll-out kernel knows of it.
 * State on the handle (allocated by init; written with ordinary stores or atomics):
 *   buf_key [Q] u32  ring of replay keys: entry number i since the last clear lives at i % Q
 *   count u64        entries appended since the last clear; live = min(count, Q)
 *   buf_gen u32      the generation the buffer belongs to
 *   cursor u64       log row number up to which rows were harvested
 *   slot_key [S] u32 key each pool slot was generated from;  slot_gen [S] u32 generation it was generated under (0: unknown)
 *   and the u64 counters harvested, pushed, replayed, n_missed, n_stale.
 * Generation: the host keeps gen, 1 at cagym_stream_scenarios, + 1 with every successful cagym_stream_set_params, passed to the
 *   kernels by value.  A key redrawn under another parameter set is a different scenario, so the buffer is valid for one generation:
 *   the harvest and push kernels clear it when buf_gen != gen (count = 0, buf_gen = gen), the refill treats it as empty.
 * Arming (k_replay_arm, one lane per world, at init): for j in 0 .. depth-1, e = episode[w] + j, slot = (w + e N) % S:
 *   e < next_episode[w]: slot_key = (uint32)(w + e N), slot_gen = gen; otherwise (a lapped world's slot) slot_gen = 0.  When a
 *   parameter switch preceded init (gen > 1) the ring may hold slots of an older set: every slot_gen starts as 0.  cursor = the
 *   log's head (rows logged before init ran on slots that may have been regenerated since), 0 without a log.
 * Refill with replay (k_stream_refill_replay; the un-armed launch stays k_stream_refill): windows, early exit, rasterisation and
 *   counters as there.  For each (w, e) it generates, idx = w + e N, key32 = (uint32)idx, rs = replay_seed ^ 0x9E3779B97F4A7C15:
 *   u0 = u(rs, key32, 0), u1 = u(rs, key32, 1) (the generator of cagym_generate_scenarios);
 *   replay iff live > 0 && buf_gen == gen && u0 < p (fp64); then j = min(live - 1, (int)(u1 * live)),
 *   key = buf_key[(count - live + j) % Q]; otherwise key = key32.  The slot (uint32)(idx % S) gets the scenario of `key`;
 *   slot_key[slot] = key, slot_gen[slot] = gen; `replayed` grows by one atomic per wave.
 *   With p == 0 or an empty buffer the pool, the steps and the log are bitwise the plain stream's.
 * Harvest (k_replay_harvest, ONE workgroup of 1024 lanes): log rows [max(cursor, head - capacity_log), head) in ascending row number;
 *   n_missed += rows overwritten before it saw them; a row (world, episode) maps to slot = (world + episode N) % S and is accepted
 *   iff (outcome & mask) != 0 && slot_gen[slot] == gen; a row whose slot_gen is neither 0 nor gen counts in n_stale; accepted rows
 *   append slot_key[slot] in row order; then cursor = head.  Enqueue it behind cagym_episode_log_update and before
 *   cagym_stream_refill (it reads slot_key of the slot the refill regenerates next - the contract the log has).  A replayed key that
 *   fails again is appended again: duplicates weigh it up; a success removes nothing.  Clearing the log restarts cursor at 0.
 * Episode log: while replay is armed the log's key column holds slot_key of the slot the episode ran on instead of w + e N - also
 *   under lapping it names the scenario that actually ran.  Without replay the log is unchanged.
 * cagym_stream_replay_init: allocates and arms (p = 0, mask = 0).  A second call clears the buffer and the counters and may change
 *   the capacity; the per-slot tables stay.  CAGYM_E_STATE when not streaming, CAGYM_E_UNSUPPORTED on an exploration stream,
 *   CAGYM_E_INVALID for capacity < 1.
 * cagym_stream_replay_set: host only, takes effect at the next launch.  p in [0, 1]; outcome_mask holds bits of the log's outcome
 *   (1 collision, 2 all at goal, 4 stuck), 0 = harvest nothing.  CAGYM_E_INVALID otherwise, CAGYM_E_STATE when not armed.
 * cagym_stream_replay_push: keys [n] u32 is a DEVICE pointer; appends in order under the current gen (one launch).
 * cagym_stream_replay_harvest: one launch; CAGYM_E_STATE without an initialised log or armed replay.
 * cagym_stream_replay_get: zero-copy DEVICE views (any pointer may be NULL); words [6] u64 = count, harvested, pushed, replayed,
 *   n_missed, n_stale.  CAGYM_E_STATE before the first init; they stay readable after the stream stopped.
 * cagym_stream_refill launches the replay variant once armed.  cagym_stream_stop and every pool setter end replay with the stream; a
 * new stream starts un-armed.
 * Out of scope: exploration streams, eviction on success, priorities beyond duplicates, replay across generations. */
int cagym_stream_replay_init(void* env, int capacity, uint64_t seed, void* stream);
int cagym_stream_replay_set(void* env, double p, uint32_t outcome_mask);
int cagym_stream_replay_push(void* env, const uint32_t* keys, int n, void* stream);
int cagym_stream_replay_harvest(void* env, void* stream);
int cagym_stream_replay_get(void* env, const uint32_t** buf_key, const uint64_t** words, const uint32_t** slot_key, const uint32_t** slot_gen,
                            int* capacity);

/* ---- Exploration worlds: an IG team on fresh maps, generated and streamed on the device (csrc/cagym_explore.h) ---------------------
 * A world holds a team of R = n_robots IG robots (CAGYM_POL_IGMCTS, FirstOrder, slots 0..R-1: the reference's ig_mcts indexes the
 * team by slot) and T = n_targets static targets (slots R..R+T-1) among the rectangles of train_stage_1 / train_stage_2.
 * The scenario of stream key v is cagym_generate_reference_scenarios' scenario of key v for the parameter set
 *   number_of_agents = R + T, fixed_count = 1, ego_policy = IGMCTS, ego_dynamics = FIRSTORDER, override_policies = 1,
 *   policy_a = policy_b = STATIC, p_b = 0, other_dynamics = FIRSTORDER, and the caller's seed, kinds_mask, n_obst_*, max_tries
 * - the same draws in the same order, nothing new is drawn - followed by the team edit of its row: slots 0..R-1 get IGMCTS,
 * FirstOrder and pref_speed = robot_pref_speed (which only sets the robots' time limit 3 (|p - g| - 0.75) / pref_speed), slots
 * R..R+T-1 get Static and radius = target_radius (IG_agent_crossing uses 0.2, tc.py:3236-3237).  Starts and goals stay as the stage
 * rule places them (1 m clear of every rectangle, 1.5 m apart); rectangles, RVO prep rows and rasters are built as there.
 * cagym_generate_exploration_scenarios: CAGYM_E_INVALID for a mask that is empty or holds another bit than the two stage kinds',
 *   n_robots < 1, n_targets < 0, n_robots + n_targets < 2 or > max_agents, a target_radius or robot_pref_speed that is not positive
 *   and finite, and whatever cagym_generate_reference_scenarios refuses of the internal set (max_tries, the stage ranges against the
 *   bounds and max_obstacles); CAGYM_E_UNSUPPORTED on a handle with max_obstacles == 0.  A refused call leaves the handle as it was.
 *   An accepted one commits the handle as cagym_generate_reference_scenarios does, except that the pool's IG robot count is known:
 *   cagym_ig_robot_inputs / _actions accept n_robots = R.  On a handle cagym_ig_init has set up it rebuilds every slot's distance
 *   field itself (the two EDT launches over S; beliefs and planner state are the caller's to restart).
 * cagym_stream_exploration_scenarios: cagym_stream_scenarios' ring contract exactly (S % N == 0, S >= 2 N, slot (w + e N) % S holds
 *   the scenario of key (uint32_t)(w + e N), the first fill equals cagym_generate_exploration_scenarios bit for bit, the counters of
 *   cagym_stream_get restart, CAGYM_E_STATE with episode records initialised).  A handle with information-gain state is accepted:
 *   the fill is followed by the rebuild of every field.  From then on cagym_stream_refill launches the exploration refill kernel
 *   (k_stream_refill's windows and counters plus the team edit) and, once cagym_ig_init has run, the FIELD REFRESH behind it:
 *   when the call returns - in stream order - edf_d2[s] is the exact squared-distance transform of the raster of every pool slot s.
 *   field_next[w] is the first episode of world w whose slot has been regenerated but not rebuilt; behind a refill the world's
 *   window is episodes max(field_next[w], episode[w] + 1) .. next_episode[w] - 1, then field_next[w] = next_episode[w]; the slot of
 *   a world's current episode is never written; fields_built counts the rebuilt slots since the stream started.
 *   Launches per cagym_stream_refill on this stream: 1 before cagym_ig_init, 4 after it (refill; work list; EDT columns; EDT rows -
 *   fixed grids striding over the device-built list), no host synchronisation, no allocation.  A refill after which no world
 *   finished costs the refresh a few loads per workgroup.  The kernels coordinate through the launch boundaries only.
 * cagym_ig_init on this stream (refused on a cagym_stream_scenarios one): builds all S fields and arms the refresh,
 *   field_next[w] = next_episode[w].
 * cagym_stream_set_exploration_params: the curriculum switch, as cagym_stream_set_params (same validation as the stream's start;
 *   takes effect for the slots later refills generate).  n_robots must stay what the stream started with (CAGYM_E_INVALID): every
 *   slot of the ring holds the same team.  CAGYM_E_STATE on a handle that streams no exploration worlds.
 * cagym_explore_stream_get: zero-copy DEVICE views field_next [N] i32 and fields_built u64 (either pointer may be NULL);
 *   CAGYM_E_STATE before the first cagym_stream_exploration_scenarios.  cagym_stream_ptrs / cagym_stream_get keep their fields.
 * Still refused while this stream runs: cagym_restore / cagym_fork, cagym_episode_records_init, and cagym_stream_set_params with
 *   the cagym_gen2_params struct (CAGYM_E_UNSUPPORTED).  cagym_stream_stop and the pool setters end it as they end any stream; the
 *   fields stay valid for the pool as it stands.
 * Out of scope: streaming a host-uploaded IG pool, snapshots of an attached planner, per-robot beliefs, a linear-time EDT. */
struct cagym_explore_params {
    uint64_t seed;
    uint32_t kinds_mask;          /* (1 << CAGYM_GEN_STAGE_1) and / or (1 << CAGYM_GEN_STAGE_2) only */
    int32_t n_robots, n_targets;  /* R >= 1, T >= 0, 2 <= R + T <= max_agents */
    int32_t n_obst_min, n_obst_max, max_tries; /* as cagym_gen2_params */
    double target_radius;
    double robot_pref_speed;
};
typedef struct cagym_explore_params cagym_explore_params;  /* (declared as cagym_stream_ptrs is) */
int cagym_generate_exploration_scenarios(void* env, const cagym_explore_params* params, int32_t* n_failed_host, void* stream);
int cagym_stream_exploration_scenarios(void* env, const cagym_explore_params* params, int32_t* n_failed_host, void* stream);
int cagym_stream_set_exploration_params(void* env, const cagym_explore_params* params);
int cagym_explore_stream_get(void* env, const int32_t** field_next, const uint64_t** fields_built);

/* ---- Terminal observations and a trajectory ring under auto-reset (csrc/cagym_terminal.h) -------------------------------------------
 * cagym_step_autoreset writes the first observation of the new episode over the one the agents ended on (DummyVecEnv hands that one
 * to the learner as infos[i]["terminal_observation"]) and restarts the state, so the last row of every agent's global_state_history
 * (agent.py:80-84, 198-201) is gone when the launch returns.  cagym_step followed by cagym_reset(mask = game_over, advance_episode)
 * equals the auto-resetting launch bit for bit - outputs, state and episode statistics (tests/test_hip_parity.py, tests/test_cfg4.py)
 * - and between those two launches both still exist.  No step, reset or roll-out kernel knows of any of this.
 * cagym_step_autoreset_keep: cagym_step_autoreset's results in `out` and in the handle, as THREE launches chained by stream order:
 *   1. the step without auto-reset, writing `out` (reward / flags / game_over are the terminal ones, as cagym_step_autoreset's);
 *   2. k_terminal_capture: for every world whose game_over byte is set, its rows of out->obs_oas / obs_ego / laserscan are copied to
 *      the same world index of `term` (rows of other worlds are NOT touched); with a trajectory ring initialised, one slice is added;
 *   3. the reset kernel for mask = out->game_over with advance_episode, writing only the restarted worlds' observations into `out`
 *      (with cfg.laserscan the on-demand scan follows, as in cagym_reset).  Unlike cagym_reset it enqueues no recorder restart: the
 *      episodes ended properly, and the episode records / log are fed from `out` exactly as behind cagym_step_autoreset.
 *   term: caller-owned DEVICE buffers shaped like their cagym_outputs counterparts; any pointer, or term itself, may be NULL.  A row is
 *   copied where both the `out` and the `term` pointer are given.  out->game_over == NULL: a handle-owned [N] scratch takes its place.
 *   No argument advances on the host: the call can be captured in a graph.  Generation-3 handles only (CAGYM_E_UNSUPPORTED).
 * The trajectory ring: a dense, handle-owned ring of L = n_slices step slices, one per cagym_step_autoreset_keep:
 *   rows [L][13][N*M] f64 in COLUMN PLANES (a wave's stores are contiguous), columns t_before, px, py, gx, gy, radius, pref_speed, vx,
 *   vy, speed, heading, a0, a1 - the reference's row, read AFTER the move with the time stamp of before it; moved [L][N*M] u8: the agent
 *   took this step (step_num advanced; rows of agents that did not move are stale); episode [L][N] i32: the episode index the world was
 *   on; last [L][N] u8: that step's game_over; head, one u64: slices ever written, slice i lives at i % L; desync, one i32.
 *   Running, the ring's own: t_prev [N,M] f64 and seen [N,M] i32, the t and step_num of every agent when the ring last saw it.
 *   CONTRACT: fed by cagym_step_autoreset_keep only, every step exactly once and in order.  A step taken through any other entry goes
 *   past the ring: the next slice finds agents whose step_num is not seen + 1, adds 1 to desync per such agent and resynchronises.
 * cagym_trajectory_init: allocate and clear; t_prev / seen are taken from the current state, so a ring attached in mid-episode starts
 *   there.  A second call clears again and may change n_slices (that synchronises the device and frees the old ring).  CAGYM_E_NOMEM
 *   when the ring does not fit.
 * cagym_trajectory_restart: the masked worlds (DEVICE [N] u8, NULL = all) take t_prev / seen from the current state; clear != 0 also
 *   zeroes every slice, head and desync.
 * cagym_trajectory_get: zero-copy DEVICE views, owned by the handle (the ring's views change when init changes n_slices).
 * Once initialised: a successful cagym_reset enqueues the restart for its mask (the abandoned episode keeps its rows and has no `last`
 * slice); a successful pool setter (cagym_set_scenarios, cagym_generate_*, cagym_stream_*scenarios) restarts every world and keeps the
 * rows.  cagym_restore and cagym_fork return CAGYM_E_STATE while a ring is initialised (its running values would describe another
 * timeline, as the log's would); cagym_snapshot stays allowed.  Handles that never called init behave as before.
 * Errors: CAGYM_E_INVALID for a NULL env; CAGYM_E_STATE before a pool is installed, and for restart / get before init;
 * CAGYM_E_UNSUPPORTED on a handle that does not run the generation-3 kernels; CAGYM_E_INVALID for n_slices < 1 or a NULL cagym_trajectory_ptrs;
 * CAGYM_E_DEVICE as every launching entry. */
struct cagym_terminal_outputs {
    float* obs_oas;   /* [N, M, M-1, 10] f32 */
    float* obs_ego;   /* [N, M, 12]      f32 */
    float* laserscan; /* [N, M, 16]      f32 (only when cfg.laserscan) */
};
typedef struct cagym_terminal_outputs cagym_terminal_outputs; /* (declared as cagym_stream_ptrs is) */
struct cagym_trajectory_ptrs {
    const double* rows;
    const uint8_t* moved;
    const int32_t* episode;
    const uint8_t* last;
    const uint64_t* head;
    const int32_t* desync;
    const double* t_prev;
    const int32_t* seen;
    int32_t n_slices;
};
typedef struct cagym_trajectory_ptrs cagym_trajectory_ptrs;
int cagym_step_autoreset_keep(void* env, const float* ext_actions, const cagym_outputs* out, const cagym_terminal_outputs* term,
                              void* stream);
int cagym_trajectory_init(void* env, int n_slices, void* stream);
int cagym_trajectory_restart(void* env, const uint8_t* world_mask, int clear, void* stream);
int cagym_trajectory_get(void* env, cagym_trajectory_ptrs* out);

/* ---- Whole-handle checkpoint: state, pool, stream, episode log and replay buffer (csrc/cagym_checkpoint.h) ---------------------------
 * cagym_restore / cagym_fork move SOME worlds onto another timeline and therefore refuse a streaming handle and an initialised log.
 * A checkpoint moves the WHOLE handle: it carries everything a run of cagym_stream_scenarios + cagym_stream_set_params +
 * cagym_episode_log_init + cagym_stream_replay_init depends on, and a load puts a fresh handle of the same configuration, or the same
 * handle, back on the same timeline bit for bit (a slot is a pure function of parameter set and key, the replay draw of seed, key, p
 * and buffer, the harvest works in row order, the counters are integer sums).  A handle that is not streaming may be checkpointed
 * too: its pool then travels with the checkpoint instead of being installed again by hand.
 * A checkpoint is two caller-owned buffers:
 *   the HOST header, sizes[CAGYM_CKPT_HOST] bytes that begin {magic u32, version u32, sizes u64 [CAGYM_CKPT_SECTIONS]} and are opaque
 *     from there on: every cagym_config field except `device`,
 *     and the host-side members the pool setters, cagym_stream_scenarios, cagym_stream_set_params, cagym_stream_replay_init / _set and
 *     cagym_episode_log_init set: pool installed, headings in use, the RVO / IG flags, streaming, the stream's parameter set and
 *     parameter generation, replay armed with p, mask, seed and capacity, log initialised with its capacity;
 *   the DEVICE blob, 16-byte aligned: the sections CAGYM_CKPT_STATE .. CAGYM_CKPT_REPLAY back to back in enum order, each a multiple
 *     of 16 bytes (0: absent).  STATE: cagym_snapshot's rows of all N worlds.  POOL: one row per scenario slot, a header {slot,
 *     CAGYM_CKPT_ROW_MAGIC, 0, 0} and the pool arrays cagym_fork copies except the raster (12 KB per slot, a pure function of the
 *     rectangles: the load rasterizes again; the rectangles' prepared RVO form is copied).  STREAM (while streaming): generated,
 *     n_failed, n_lapped, next_episode [N].  LOG (once initialised): every ring column, the running arrays, the slice counter and
 *     head.  REPLAY (while armed): buf_key [Q], the counters and the harvest cursor, the buffer's generation, slot_key / slot_gen [S].
 * cagym_checkpoint_sizes: sizes[CAGYM_CKPT_SECTIONS] of the handle as it is now; host only.
 * cagym_checkpoint_save: writes the header into host_words before it returns and enqueues three copy launches into `blob` on `stream`
 *   (rows of worlds, rows of slots, one flat copy of the other sections).  Nothing moves: a pending cagym_step_begin stays valid.
 * cagym_checkpoint_load: validates the header on the host before anything is enqueued - magic, version, host_bytes, the section sizes
 *   (against blob_bytes and against what this handle holds for the header's capacities), every config field except `device`, and the
 *   header's members as the calls that set them do; any mismatch is CAGYM_E_INVALID and leaves the handle untouched.  Then the
 *   handle's stream, log and replay state become the checkpoint's: streaming starts or ends, log and replay are initialised, a ring
 *   whose capacity differs is allocated again (that synchronises the device, as a second cagym_episode_log_init does; nothing is
 *   allocated where the capacities match), a log the checkpoint lacks is cleared as cagym_episode_log_restart(NULL, 1) clears it, and
 *   the three copies and the raster launch are enqueued on `stream`.  A pending cagym_step_begin is void afterwards.  The caller's
 *   output buffers are not part of a checkpoint.  The blob is trusted as cagym_restore trusts its own: a row without its magic, or
 *   with an id out of range, is skipped on the device; the counters and keys are taken as they are.
 *   After CAGYM_E_NOMEM / CAGYM_E_HIP from a load the handle's pool, log and replay contents are unspecified: load again or install a pool.
 * Errors, in this order: CAGYM_E_INVALID for a NULL env; CAGYM_E_STATE for sizes / save before a pool is installed;
 * CAGYM_E_UNSUPPORTED on an exploration stream and after cagym_ig_init (per-slot distance fields and planner workspaces are not
 * carried); CAGYM_E_STATE with an initialised trajectory ring or initialised episode records; CAGYM_E_INVALID for a NULL sizes /
 * host_words / blob, a blob that is not 16-byte aligned, buffers smaller than cagym_checkpoint_sizes says, and what load validates;
 * CAGYM_E_DEVICE as every launching entry.  cagym_restore and cagym_fork keep their refusals. */
#define CAGYM_CKPT_MAGIC 0x43474B31u     /* "CGK1" */
#define CAGYM_CKPT_ROW_MAGIC 0x43475031u /* "CGP1": a pool row of the blob */
#define CAGYM_CKPT_VERSION 1
enum { CAGYM_CKPT_HOST = 0, CAGYM_CKPT_STATE = 1, CAGYM_CKPT_POOL = 2, CAGYM_CKPT_STREAM = 3, CAGYM_CKPT_LOG = 4, CAGYM_CKPT_REPLAY = 5,
       CAGYM_CKPT_SECTIONS = 6 };
int cagym_checkpoint_sizes(void* env, uint64_t* sizes);
int cagym_checkpoint_save(void* env, void* host_words, uint64_t host_bytes, void* blob, uint64_t blob_bytes, void* stream);
int cagym_checkpoint_load(void* env, const void* host_words, uint64_t host_bytes, const void* blob, uint64_t blob_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
