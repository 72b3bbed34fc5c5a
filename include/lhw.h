/* lhw.h -- C ABI of the MI355X-native batched environment stepper + PPO update
 * (liblhw.so, built from learninghumanoidwalking_amd/csrc for gfx950).
 *
 * This is the drop-in boundary of the hot path.  The reference has
 * no FFI of its own -- it is pure Python over third-party wheels -- so each entry point
 * below names the reference interface whose work it takes over:
 *
 *   lhw_env_create   <- env_fn() / BaseHumanoidEnv.__init__ + MujocoEnv.__init__
 *                       (reference envs/common/base_humanoid_env.py:38-74,
 *                        envs/common/mujoco_env.py:16-36, envs/cartpole/cartpole_env.py:82-107)
 *   lhw_env_reset    <- MujocoEnv.reset -> reset_model
 *                       (envs/common/mujoco_env.py:113-116, base_humanoid_env.py:247-276,
 *                        envs/cartpole/cartpole_env.py:109-121)
 *   lhw_env_step     <- env.step(action) for every env of the batch, plus the per-step episode
 *                       bookkeeping of RolloutWorker.sample (truncation at max_traj_len,
 *                       terminal observation for the bootstrap value, reset on episode end)
 *                       (base_humanoid_env.py:199-227, robots/robot_base.py:41-98,
 *                        envs/common/robot_interface.py:493-546 [PD + mj_step],
 *                        rl/workers/rollout_worker.py:142-181)
 *   lhw_env_get_state / lhw_env_set_state
 *                    <- data.qpos / data.qvel reads, MujocoEnv.set_state
 *                       (envs/common/mujoco_env.py:118-127); parity hooks
 *   lhw_env_set_iteration <- RolloutWorker.sync_state's env.robot.iteration_count = itr
 *                       (rl/workers/rollout_worker.py:95)
 *   lhw_env_*task_inputs, lhw_env_*step_task_inputs
 *                    <- what RobotBase.step hands the exchangeable task once per control step
 *                       (robots/robot_base.py:88-96: task.step / calc_reward / done reading RobotInterface);
 *                       the second record adds what SteppingTask reads besides (tasks/stepping_task.py:66-123, 209-262)
 *   lhw_gae          <- PPOBuffer.finish_path over every trajectory of the batch
 *                       (rl/storage/rollout_storage.py:53-85)
 *   lhw_mlp_*, lhw_ppo_* <- Gaussian_FF_Actor / FF_V forward and PPO.update_actor_critic
 *                       (rl/policies/actor.py:160-188, rl/policies/critic.py:41-49,
 *                        rl/algos/ppo.py:299-406)
 *
 * Conventions: every function returns 0 on success or a negative LhwStatus; the message is
 * available from lhw_last_error().  The caller owns every buffer and passes raw device (or,
 * where stated, host) pointers -- no torch types cross this boundary.  `stream` is a
 * hipStream_t passed as void* (NULL = the default stream); calls are asynchronous with respect
 * to it unless stated.  One handle belongs to one device and one host thread at a time.
 */
#ifndef LHW_H
#define LHW_H

#include <stdint.h>

#include "lhw_model_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  LHW_OK = 0,
  LHW_ERR_ARG = -1,         /* bad argument / size mismatch */
  LHW_ERR_HIP = -2,         /* HIP runtime error (message has hipGetErrorString) */
  LHW_ERR_MODEL = -3,       /* model blob malformed or exceeds a compiled-in limit */
  LHW_ERR_UNSUPPORTED = -4, /* feature outside the implemented subset */
  LHW_ERR_NO_DEVICE = -5    /* no usable GPU: the product path has no CPU fallback */
} LhwStatus;

typedef enum {
  LHW_TASK_CARTPOLE = 0, /* reference envs/cartpole/cartpole_env.py */
  LHW_TASK_JVRC_WALK = 1, /* reference envs/jvrc/jvrc_walk.py + tasks/walking_task.py */
  LHW_TASK_H1_STAND = 2,  /* reference envs/h1/h1_env.py + tasks/standing_task.py (+ domain_randomization.py) */
  LHW_TASK_JVRC_STEP = 3, /* reference envs/jvrc/jvrc_step.py + tasks/stepping_task.py (box terrain, footstep targets) */
  LHW_TASK_H1_WALK = 4    /* reference envs/h1/h1_walk.py: H1 robot (noise, randomisation as H1_STAND) + tasks/walking_task.py;
                             task_params / task_iparams as LHW_TASK_H1_STAND, plus clock_lut / period */
} LhwTask;

/* done flags written by lhw_env_step */
#define LHW_DONE_TERMINATED 1u /* env.step returned done=True */
#define LHW_DONE_TRUNCATED 2u  /* trajectory reached max_traj_len (rollout_worker.py:152) */

typedef struct LhwEnv LhwEnv;

typedef struct {
  int32_t task;         /* LhwTask */
  int32_t n_envs;       /* batch size N */
  int32_t device;       /* HIP device ordinal */
  int32_t frame_skip;   /* sim sub-steps per control step (control_dt / sim_dt) */
  int32_t max_traj_len; /* >0: truncate + auto-reset like RolloutWorker.sample; 0: never reset inside step */
  int32_t env_id_base;  /* global index of env 0 (RNG keys use env_id_base + n): multi-GPU sharding */
  uint64_t seed;        /* counter-based RNG key (replaces the reference's global np.random stream) */
  double action_smoothing;       /* base_humanoid_env.py:209 (unused by cartpole) */
  const double* kp;              /* [nu] PD gains */
  const double* kd;              /* [nu] */
  const double* nominal_qpos;    /* [nq] reset pose (jvrc_base.py:52-54); NULL -> qpos0 */
  const double* action_offset;   /* [nu] nominal joint pose added to targets (base_humanoid_env.py:212) */
  const double* task_params;     /* task-specific doubles, see LHW_TP_* */
  int32_t n_task_params;
  const int32_t* task_iparams;   /* task-specific ints, see LHW_TI_* */
  int32_t n_task_iparams;
  const double* clock_lut;       /* walking: [4][period] r_frc, r_vel, l_frc, l_vel at integer phases
                                    (tasks/rewards.py:196-300 evaluated on 0..period-1) */
  int32_t period;
  double init_noise;             /* BaseHumanoidEnv._apply_init_noise (envs/common/base_humanoid_env.py:278-305) for ANY humanoid task: half-width in
                                    radians of the uniform noise on root roll / pitch and every joint at reset (root z += U(0, 0.02)); 0 = off.
                                    (H1 tasks may also give it as task_params[LHW_TP_H1_INIT_NOISE]; this field wins when > 0.) */
  /* apply_perturbation for the JVRC tasks (envs/common/domain_randomization.py:10-26 behind base_humanoid_env.py:86-92, 224-225; the H1 tasks
   * carry theirs in task_params / task_iparams): after the observation of a control step, with probability 1 / interval, every listed body
   * receives a world-frame force U(+-force)^3 and torque U(+-torque)^3 at its centre of mass, each body followed by a coin flip that clears ALL
   * applied wrenches; they act until the next draw or reset.  interval = int(cfg.interval / control_dt) control steps, 0 = off. */
  int32_t perturb_interval;
  int32_t n_perturb_bodies;      /* <= 2 */
  int32_t perturb_bodies[2];     /* body ids of the packed model */
  double perturb_force, perturb_torque;
} LhwEnvConfig;

/* task_params indices: [0] target root height (walking goal_height / standing 0.98); H1 standing adds the
 * init-noise half-width (rad), perturbation force / torque magnitudes and 35 per-entry observation-noise half-widths */
enum { LHW_TP_GOAL_HEIGHT = 0, LHW_TP_COUNT = 1, LHW_TP_H1_INIT_NOISE = 1, LHW_TP_H1_FORCE_MAG = 2, LHW_TP_H1_TORQUE_MAG = 3,
       LHW_TP_H1_OBS_NOISE = 4 };
/* stepping task: local offsets of the right / left foot force sites on the foot bodies, target radius
 * (stepping_task.py:268), half sizes of the terrain boxes (:325), then the footstep plans of the CURVED mode:
 * count, and per plan 1 + 20*3 doubles = length, (x, y, theta) rows (stepping_task.py:52-64) */
enum { LHW_TP_STEP_RSITE = 1, LHW_TP_STEP_LSITE = 4, LHW_TP_STEP_RADIUS = 7, LHW_TP_STEP_BOX_SIZE = 8, LHW_TP_STEP_NPLANS = 11,
       LHW_TP_STEP_PLANS = 12, LHW_STEP_MAX_SEQ = 20 };
/* task_iparams indices: body ids of root, head (walking) / torso (standing), right foot, left foot; H1 standing adds the
 * randomisation intervals in control steps, the perturbed bodies, and the randomised dofs (10) and bodies (11) */
enum { LHW_TI_ROOT_BODY = 0, LHW_TI_HEAD_BODY = 1, LHW_TI_RFOOT_BODY = 2, LHW_TI_LFOOT_BODY = 3, LHW_TI_COUNT = 4,
       LHW_TI_H1_DYNRAND_INTERVAL = 4, LHW_TI_H1_PERTURB_INTERVAL = 5, LHW_TI_H1_N_PBODY = 6, LHW_TI_H1_PBODY = 7,
       LHW_TI_H1_RAND_DOF = 9, LHW_TI_H1_RAND_BODY = 19 };
/* stepping task: first terrain-box geom id (boxes are contiguous), box count (<= 20), floor geom id, target dwell in
 * control steps (stepping_task.py:269) */
enum { LHW_TI_STEP_BOX_GEOM0 = 4, LHW_TI_STEP_NBOX = 5, LHW_TI_STEP_FLOOR_GEOM = 6, LHW_TI_STEP_DELAY_FRAMES = 7, LHW_TI_STEP_COUNT = 8 };

int lhw_version(void);
const char* lhw_last_error(void);

/* model_i / model_d: packed model blobs (host pointers), layout in lhw_model_fields.h */
int lhw_env_create(const int32_t* model_i, int64_t n_model_i, const double* model_d, int64_t n_model_d,
                   const LhwEnvConfig* cfg, LhwEnv** out);
int lhw_env_destroy(LhwEnv* env);

int lhw_env_obs_dim(const LhwEnv* env);
int lhw_env_act_dim(const LhwEnv* env);
int lhw_env_num_reward_terms(const LhwEnv* env);
int lhw_env_nq(const LhwEnv* env);
int lhw_env_nv(const LhwEnv* env);

/* Reset the envs whose mask byte is non-zero (mask_dev == NULL: all).  obs_dev [N][obs_dim] f32
 * receives the first observation of the reset envs (rows of other envs are left untouched). */
int lhw_env_reset(LhwEnv* env, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* One control step for all N envs.
 *   act_dev      [N][act_dim] f32, in
 *   obs_dev      [N][obs_dim] f32, out: observation to act on next (after the auto-reset, if any)
 *   term_obs_dev [N][obs_dim] f32, out, nullable: observation returned by env.step itself
 *                (differs from obs_dev only where the episode ended: bootstrap input)
 *   rew_dev      [N] f32, out: sum of reward terms in the reference's dict order
 *   done_dev     [N] u8, out: LHW_DONE_* flags
 *   rew_terms_dev [N][num_reward_terms] f32, out, nullable */
int lhw_env_step(LhwEnv* env, const float* act_dev, float* obs_dev, float* term_obs_dev, float* rew_dev,
                 uint8_t* done_dev, float* rew_terms_dev, void* stream);

/* Test hook: copy the per-env stepping-task record to host: seq [N][20][6] = (x y z theta cos sin) of every target step /
 * terrain box, floor_z [N], and istate [N][5] = t1 t2 target_reached target_reached_frames sequence_length. */
int lhw_env_debug_step_record(LhwEnv* env, double* seq, double* floor_z, int32_t* istate);

/* Same as lhw_env_step for the envs [first, first + count) only; all pointers are the FULL-batch arrays (the range indexes
 * into them).  Lets the host pipeline independent groups of envs on separate HIP streams: without a batch-wide barrier per
 * control step, the tail of one group's kernel overlaps the next group's (wave-per-env steppers only). */
int lhw_env_step_range(LhwEnv* env, int32_t first, int32_t count, const float* act_dev, float* obs_dev, float* term_obs_dev,
                       float* rew_dev, uint8_t* done_dev, float* rew_terms_dev, void* stream);
/* The frozen actor as the resident rollout evaluates it inside the stepper's wavefronts: the reference's worker holds a copy of
 * the policy for the whole rollout (rl/workers/rollout_worker.py:62-77 sync_policy) and calls it once per control step
 * (:142-150, Gaussian_FF_Actor.forward rl/policies/actor.py:160-188).  Device pointers, filled by lhw_ppo_rollout_policy. */
typedef struct {
  const float *w1t, *b1, *w2t, *b2, *w3t, *b3; /* TRANSPOSED weights ([in][out]: W1^T [obs_pad][hidden], W2^T [hidden][hidden],
                                                  W3^T [hidden][act_pad]) and the biases */
  const float *stdv;                           /* [act_dim] standard deviations of the Gaussian head */
  const float *obs_mean, *obs_std;             /* [obs_dim] observation normalisation (actor.obs_mean / obs_std) */
  int32_t obs_dim, obs_pad, act_dim, act_pad, hidden;
  int32_t deterministic;                       /* != 0: act = mean (evaluation) */
  int32_t fp16_operands;                       /* != 0: weights and activations rounded to fp16 per product, float32 accumulation
                                                  (lhw_ppo_set_inference_dtype; BASELINE config 5 "fp16 actor / critic") */
  uint64_t seed;                               /* policy-noise key, as lhw_ppo_forward's */
  uint32_t counter;                            /* policy-stream counter of the FIRST control step; step t uses counter + t */
} LhwRolloutPolicy;
/* The resident rollout: T control steps of envs [first, first + count) in ONE launch -- the body of RolloutWorker.sample's loop
 * (rl/workers/rollout_worker.py:142-181: action = policy(state); env.step(action); store; reset on episode end) executed wave
 * by wave, no wavefront ever waiting for another env's control step.  Bitwise the values of T x { lhw_ppo_forward_at(act, logp
 * only) ; lhw_env_step_range } on the same buffers.  All pointers are device buffers, TIME-major over the FULL batch (N = the
 * env's n_envs; the range indexes into each time slice):
 *   obs_dev      [T + 1][N][obs_dim] f32: slice 0 in (the observation to act on first: lhw_env_reset's output or slice T of the
 *                previous rollout), slices 1 .. T out
 *   act_dev      [T][N][act_dim], logp_dev [T][N]: sampled actions and their log-densities, out
 *   term_obs_dev [T][N][obs_dim], rew_dev [T][N], done_dev [T][N] (LHW_DONE_*): as lhw_env_step, per control step, out
 *   rew_terms_dev [N][num_reward_terms] of the LAST control step, nullable
 * Humanoid tasks only, feed-forward float32 actor with hidden width 256 and act_dim <= 12 (LHW_ERR_UNSUPPORTED otherwise: the
 * caller keeps the launch-per-step pipeline).  Ranges of concurrent calls on different streams must be disjoint.  Stepping task
 * with more envs than the chip has wave slots: the resident wavefronts drain a device queue of (env, LHW_ROLLOUT_CHUNK = 10 control
 * steps) jobs instead of keeping one env each (the cost of an env follows its walking mode; same values either way). */
int lhw_env_rollout(LhwEnv* env, const LhwRolloutPolicy* policy, int32_t first, int32_t count, int32_t T, float* obs_dev, float* act_dev,
                    float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev, float* rew_terms_dev, void* stream);
/* lhw_env_rollout that also exports the batched sim facade (below) of EVERY control step: tin_dev [T][N][LHW_TASK_INPUT_DIM] float64
 * receives, per control step and env, the record lhw_env_get_task_inputs would return after that step -- what the reference's robot
 * hands its exchangeable task once per control step (robots/robot_base.py:88-96: task.step / calc_reward / done reading RobotInterface).
 * For task code that only changes the REWARD (an edited tasks/rewards.py): the rollout runs resident with the fused termination and
 * resets, and the plug-in evaluates the whole [T * N] batch once after the launch (task_hook.py).  Everything else as lhw_env_rollout. */
int lhw_env_rollout_task_inputs(LhwEnv* env, const LhwRolloutPolicy* policy, int32_t first, int32_t count, int32_t T, float* obs_dev,
                                float* act_dev, float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev, float* rew_terms_dev,
                                double* tin_dev, void* stream);
/* The frozen LSTM actor (Gaussian_LSTM_Actor, rl/policies/actor.py:191-286: two stacked LSTMCells of `hidden` units and a linear
 * read-out) as lhw_env_rollout_lstm evaluates it inside the stepper's wavefronts -- the reference's worker calls it once per control
 * step and carries its hidden / cell state from step to step, zeroed where an episode starts (rl/workers/rollout_worker.py:130-190).
 * Device pointers, filled by lhw_rnn_rollout_policy. */
typedef struct {
  const float *w1t, *bi1, *bh1;      /* W1cat^T [obs_pad + hidden][4 hidden]: the TRANSPOSED [W_ih | W_hh] of cell 1 (rows in the order of the
                                        concatenated input [x | h1_prev], padded observation columns included; columns gate-major i f g o),
                                        and its two bias vectors [4 hidden] */
  const float *w2t, *bi2, *bh2;      /* W2cat^T [2 hidden][4 hidden] (input [h1 | h2_prev]) and the biases of cell 2 */
  const float *wot, *bo;             /* Wout^T [hidden][act_pad] and the read-out bias */
  const float *stdv;                 /* [act_dim] standard deviations of the Gaussian head */
  const float *obs_mean, *obs_std;   /* [obs_dim] observation normalisation */
  float *h1, *h2, *c1, *c2;          /* the recurrent state, READ AND WRITTEN, one row per env of the batch: hidden states with row strides
                                        h1_ld / h2_ld floats, cell states [state_rows][hidden].  For an LhwRnn handle these are its own actor
                                        state buffers, the ones lhw_rnn_forward(commit = 1) advances */
  int32_t h1_ld, h2_ld, state_rows;
  int32_t obs_dim, obs_pad, act_dim, act_pad, hidden;
  int32_t deterministic;             /* != 0: act = mean (evaluation) */
  uint64_t seed;                     /* policy-noise key, as lhw_rnn_forward's */
  uint32_t counter;                  /* policy-stream counter of the FIRST control step; step t uses counter + t */
} LhwRolloutLstmPolicy;
/* lhw_env_rollout for an LSTM actor: T control steps of envs [first, first + count) in ONE launch, every wavefront evaluating the two
 * LSTM cells and the read-out for its own env(s) -- the loop of RolloutWorker.sample with a recurrent policy
 * (rl/workers/rollout_worker.py:130-190).  Bitwise the values of T x { lhw_rnn_forward(actor outputs, commit = 1) ; lhw_env_step } on the
 * same buffers, the state buffers of the view included, so rollouts of either kind may follow each other on one LhwRnn handle.  Buffers as
 * for lhw_env_rollout.  reset0_dev [N] u8: rows whose episode starts with slice 0 of obs_dev (their stored state counts as zero); at step
 * t > 0 the state is zero where done_dev[t - 1] is set.  tin_dev / stin_dev: nullable, the records of every control step as in
 * lhw_env_rollout_task_inputs / lhw_env_rollout_step_task_inputs.  Float32 LSTM actor with hidden width 256 and act_dim <= 12, a state
 * row per env of the batch (LHW_ERR_UNSUPPORTED otherwise, and wherever lhw_env_rollout refuses). */
int lhw_env_rollout_lstm(LhwEnv* env, const LhwRolloutLstmPolicy* policy, int32_t first, int32_t count, int32_t T, float* obs_dev, float* act_dev,
                         float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev, float* rew_terms_dev, const uint8_t* reset0_dev,
                         double* tin_dev, double* stin_dev, void* stream);
/* lhw_env_rollout for an env with an OBSERVATION HISTORY (obs_history_len of the reference's YAML configs,
 * envs/common/base_humanoid_env.py:53,177-197,274: the observation is the last history_len base observations, newest first, flattened; a
 * reset empties the history and zero-fills it).  obs_dev [T + 1][N][history_len * base] and term_obs_dev [T][N][history_len * base], base =
 * lhw_env_obs_dim(env); policy->obs_dim must equal history_len * base.  Slice 0 of obs_dev holds the full observations to act on first; per
 * control step the wavefront that advances an env shifts its row on the device:
 *   obs[t + 1][n] = [ base observation of step t | done[t][n] ? +0 : obs[t][n] without its last `base` columns ]
 *   term_obs[t][n] = [ terminal base observation | obs[t][n] without its last `base` columns ]
 * Nothing of the history is kept in the env handle: obs_dev is the state, slice T the input of the next rollout.  The policy step for rows
 * wider than 64 columns sums in the order of the per-layer GEMM forward the launch-per-step pipeline runs for such rows (lhw_ppo_forward_at:
 * every layer one chain over ascending k, the bias behind it); lhw_debug_policy_step is its reference, bit for bit.  tin_dev / stin_dev:
 * nullable, the records of every control step as in lhw_env_rollout_task_inputs / lhw_env_rollout_step_task_inputs.  history_len == 1
 * forwards to those entry points and launches their kernels.  LHW_ERR_UNSUPPORTED wherever lhw_env_rollout refuses, and for a padded row
 * wider than LHW_ROLLOUT_HISTORY_MAX_OBS_PAD (history_len <= 27 on jvrc_walk, 26 on jvrc_step, 29 on h1, 23 on h1_walk).  Rows wider than
 * 256 columns pass through the wave's LDS in pieces of 256; the first layer's chain of a hidden unit runs on from piece to piece, so it is
 * the same chain at every width. */
int lhw_env_rollout_history(LhwEnv* env, const LhwRolloutPolicy* policy, int32_t first, int32_t count, int32_t T, int32_t history_len,
                            float* obs_dev, float* act_dev, float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev,
                            float* rew_terms_dev, double* tin_dev, double* stin_dev, void* stream);
/* 1 if the most recent lhw_env_rollout of this env drained the job queue (rocprof name humanoid_rollout_kernel<TASK, 64, true>), 0 if
 * every wavefront kept its env group (<.., false>); what bench.py names as the dominant kernel. */
int lhw_env_last_rollout_queued(LhwEnv* env);
/* Parity hooks; HOST pointers, synchronous.  qpos [N][nq], qvel [N][nv] float64. */
int lhw_env_get_state(LhwEnv* env, double* qpos_host, double* qvel_host);
int lhw_env_set_state(LhwEnv* env, const double* qpos_host, const double* qvel_host);
/* The batched sim facade: everything the reference's tasks read through RobotInterface for one control step
 * (envs/common/robot_interface.py:75-82 qpos / qvel / qacc, :163-185 actuator position / velocity / torque, :242-250 foot body
 * positions, :269-325 foot-floor contacts and ground reaction forces, :357-380 body velocities, :382-394 object positions,
 * :472-484 self collisions) plus the arguments RobotBase.step passes to calc_reward (robots/robot_base.py:88-96), as the fused
 * kernel saw them when it evaluated the reward of the LAST control step.  Slow-path hook for task code that is not compiled
 * into the kernel (a user's BaseTask, tasks/base_task.py:12-83, or the reference's own tasks/rewards.py run as a cross-check):
 * enable once, step, then read the [N][LHW_TASK_INPUT_DIM] float64 records on the host or, for on-device consumers, through the
 * device pointer.  Derived fields follow MuJoCo's staleness (SURVEY note S): positions / velocities of bodies, contacts, qacc
 * and actuator fields describe the last forward pass, qpos / qvel the state after it. */
enum LhwTaskInput {
  LHW_TIN_GRF_R = 0,          /* get_rfoot_grf(): sum over the right foot's floor contacts of |contact wrench| */
  LHW_TIN_GRF_L = 1,
  LHW_TIN_CONTACT_Z = 2,      /* min z of the foot-floor contact points (0 when there is none) */
  LHW_TIN_FOOT_CONTACT = 3,   /* check_rfoot_floor_collision() or check_lfoot_floor_collision() */
  LHW_TIN_SELF_COLLISION = 4, /* check_self_collisions() */
  LHW_TIN_PHASE = 5,          /* task._phase, mode (WalkModes / stepping mode index) and mode_ref AFTER task.step() */
  LHW_TIN_MODE = 6,
  LHW_TIN_MODE_REF = 7,       /* 3 */
  LHW_TIN_RFOOT_VEL = 10,     /* 3: linear velocity of the body frame origin (mj_objectVelocity), world axes; the tasks use its norm */
  LHW_TIN_LFOOT_VEL = 13,     /* 3 */
  LHW_TIN_ROOT_VEL_LOCAL = 16,/* 3: get_body_vel(root, frame=1)[0] */
  LHW_TIN_ROOT_XPOS = 19,     /* 3 */
  LHW_TIN_HEAD_XPOS = 22,     /* 3 */
  LHW_TIN_RFOOT_XPOS = 25,    /* 3 */
  LHW_TIN_LFOOT_XPOS = 28,    /* 3 */
  LHW_TIN_QPOS = 32,          /* nq <= 19 */
  LHW_TIN_QVEL = 51,          /* nv <= 18 */
  LHW_TIN_QACC = 69,          /* nv */
  LHW_TIN_ACT_POS = 87,       /* nu <= 12: get_act_joint_positions() */
  LHW_TIN_ACT_VEL = 99,
  LHW_TIN_ACT_TAU = 111,      /* get_act_joint_torques() */
  LHW_TIN_PREV_TORQUE = 123,  /* calc_reward(prev_torque, prev_action, action) */
  LHW_TIN_PREV_ACTION = 135,
  LHW_TIN_ACTION = 147,
  LHW_TIN_ROOT_XMAT = 160,    /* 9: get_object_affine_by_name(root body)'s rotation, row-major (standing_task.py:76-85: the torso in the pelvis frame) */
  LHW_TASK_INPUT_DIM = 176
};
int lhw_env_enable_task_inputs(LhwEnv* env, int enable);
/* HOST pointer [N][LHW_TASK_INPUT_DIM] float64, synchronous; humanoid tasks only, after lhw_env_enable_task_inputs(env, 1). */
int lhw_env_get_task_inputs(LhwEnv* env, double* out_host);
/* The same records on the device (valid until the env is destroyed or the export disabled); NULL while disabled. */
int lhw_env_task_inputs_device(LhwEnv* env, double** out_dev);
/* The stepping task's second record (jvrc_step only): what SteppingTask.step / calc_reward / done (tasks/stepping_task.py:66-123,
 * 209-262) read besides the LhwTaskInput fields -- the foot force sites, the footstep targets and the target state machine, the root
 * quaternion -- as the fused kernel saw them for the LAST control step, after task.step() (update_target_steps included).  A stepping
 * task plugged in from outside the kernel reads this record next to the LhwTaskInput one (task_hook.py: VectorSteppingTask).  The
 * target state machine that feeds the observation stays in the kernel; the record carries its state. */
enum LhwStepTaskInput {
  LHW_STIN_RSITE_XPOS = 0,    /* 3: get_object_xpos_by_name("rf_force", OBJ_SITE) -- r_foot_pos (stepping_task.py:218), the stale site frame */
  LHW_STIN_LSITE_XPOS = 3,    /* 3: "lf_force" -- l_foot_pos (:217) */
  LHW_STIN_TARGET1 = 6,       /* 4: sequence[t1] x, y, z, theta (:67, :81, :225) after update_target_steps (:201-207) */
  LHW_STIN_TARGET2 = 10,      /* 4: sequence[t2] (:73) */
  LHW_STIN_REACHED = 14,      /* target_reached (:70, :230-234) */
  LHW_STIN_FRAMES = 15,       /* target_reached_frames (:231) */
  LHW_STIN_T1 = 16,           /* t1, t2 (:201-207) */
  LHW_STIN_T2 = 17,
  LHW_STIN_NSEQ = 18,         /* len(sequence) */
  LHW_STIN_GOAL = 19,         /* 8: update_goal_steps (:184-199): goal x[2] y[2] z[2] theta[2] in the root frame, observation order (jvrc_step.py:66-77) */
  LHW_STIN_ROOT_XQUAT = 27,   /* 4: get_object_xquat_by_name(root, OBJ_BODY) (:82), w x y z -- calc_body_orient_reward's root_quat */
  LHW_STEP_TASK_INPUT_DIM = 32   /* (31: reserved, written as 0) */
};
/* Arms (enable = 1: allocates [N][LHW_STEP_TASK_INPUT_DIM] float64, released with the env) or stops (0) the export; the launch-per-step
 * path writes it on every control step from then on.  LHW_ERR_UNSUPPORTED on an env of another task. */
int lhw_env_enable_step_task_inputs(LhwEnv* env, int enable);
/* HOST pointer [N][LHW_STEP_TASK_INPUT_DIM] float64, synchronous; after lhw_env_enable_step_task_inputs(env, 1). */
int lhw_env_get_step_task_inputs(LhwEnv* env, double* out_host);
/* The same records on the device (valid until the env is destroyed or the export disabled); NULL while disabled. */
int lhw_env_step_task_inputs_device(LhwEnv* env, double** out_dev);
/* lhw_env_rollout_task_inputs that also exports the stepping record of EVERY control step: stin_dev [T][N][LHW_STEP_TASK_INPUT_DIM]
 * float64 (jvrc_step only, LHW_ERR_UNSUPPORTED otherwise).  Everything else as lhw_env_rollout_task_inputs. */
int lhw_env_rollout_step_task_inputs(LhwEnv* env, const LhwRolloutPolicy* policy, int32_t first, int32_t count, int32_t T, float* obs_dev,
                                     float* act_dev, float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev, float* rew_terms_dev,
                                     double* tin_dev, double* stin_dev, void* stream);
/* Actuated-joint fields of the LAST forward pass, as the reference's RobotInterface getters return them after env.step
 * (envs/common/robot_interface.py:163-185: get_act_joint_positions / _velocities / _torques = actuator_length / gear,
 * actuator_velocity / gear, actuator_force * gear).  HOST pointers [N][nu] float64, synchronous; humanoid tasks only. */
int lhw_env_get_actuator_state(LhwEnv* env, double* pos_host, double* vel_host, double* torque_host);
/* Episode statistics accumulated on device since the last call: sum of finished-episode returns,
 * sum of finished-episode lengths, number of finished episodes (host pointers, synchronous, resets them). */
int lhw_env_pop_episode_stats(LhwEnv* env, double* ret_sum, double* len_sum, int64_t* count);
/* Per-term episode statistics: the reward dictionary every env.step of the reference returns as `info` (robots/robot_base.py:88-96
 * `rewards = self._task.calc_reward(...)`, `return obs, sum(rewards.values()), done, rewards`; envs/cartpole/cartpole_env.py:155-187),
 * which a batched rollout otherwise drops.  While enabled, every control step -- launch per step, resident rollout, job queue, the
 * in-wave re-run of an env with more than 8 contacts (counted once) -- adds the env's reward terms (float64, after the divergence guard)
 * to per-env episode sums kept beside the env records; the step that ends an episode (LHW_DONE_*) moves those sums to the env's
 * finished-episode sums and counts the episode as terminated (LHW_DONE_TERMINATED set) or truncated (LHW_DONE_TRUNCATED alone);
 * lhw_env_reset zeroes the running sums of the envs it resets.  Each env's row has one writer (no atomics): what a pop returns does not
 * depend on the order in which wavefronts finish.  No other output of a step changes by a bit.
 * enable = 1 allocates [N][22] float64 (released with the env) and zeroes all sums; 0 stops the accumulation. */
#define LHW_MAX_REWARD_TERMS 10 /* tasks/walking_task.py calc_reward: the longest dictionary of the implemented tasks */
int lhw_env_enable_term_stats(LhwEnv* env, int enable);
/* The sums over all envs since the last call, added up in env order (host pointers, any may be NULL; synchronous; resets the
 * finished-episode sums only -- episodes still running keep their partial sums): term_sum [lhw_env_num_reward_terms] = sum over the finished episodes of the episode's sum of each
 * term, in the reference's dict order (the order of rew_terms_dev); episodes = terminated + truncated.  LHW_ERR_ARG while disabled. */
int lhw_env_pop_term_stats(LhwEnv* env, double* term_sum, int64_t* episodes, int64_t* terminated, int64_t* truncated);
/* Task shaping: the leading weight of every reward term and the termination bounds of the fused humanoid tasks, which the reference
 * keeps as literals in tasks/walking_task.py, stepping_task.py and standing_task.py (calc_reward / done).  An env starts with the
 * reference's values; the setter replaces them for the whole batch from the next launch on, in every way a control step is executed
 * (launch per step, resident rollouts of every policy kind), with rew_terms and the per-term statistics reporting the weighted terms.
 * term_weights [n_weights = lhw_env_num_reward_terms], in the order of rew_terms_dev; finite, negative allowed (a penalty).
 * term_limits [n_limits = LHW_TERM_LIMIT_COUNT]: walking / standing terminate on root z < [0] or root z > [1]; the stepping task on
 * (root z - lower foot site z) < [0], and its [1] must be +inf.  No NaN, [0] < [1]; -inf / +inf switch a bound off.  The inner
 * constants of the terms and the self-collision rule are not settings.  HOST pointers; either may be NULL, which leaves that half as it
 * is.  Synchronises the device (as lhw_env_set_state).  Episodes in flight continue under the new values: their return, and their
 * running per-term sums, simply carry on -- a curriculum that changes weights between iterations mixes both in the episodes that span
 * the change.  LHW_ERR_ARG (nothing changed) for a wrong count or value, LHW_ERR_UNSUPPORTED for cartpole. */
#define LHW_TERM_LIMIT_COUNT 2   /* [0] lower bound, [1] upper bound (stepping task: must be +inf, it has none) */
int lhw_env_set_task_shaping(LhwEnv* env, const double* term_weights, int32_t n_weights, const double* term_limits, int32_t n_limits);
int lhw_env_get_task_shaping(const LhwEnv* env, double* term_weights /*[lhw_env_num_reward_terms]*/, double* term_limits /*[2]*/);
/* Actuator randomisation: the two sim-to-real settings of the reference's PD law (robots/robot_base.py:5-62; every humanoid env inherits
 * them), for the whole batch and, like the task shaping, from the next control step on.  Off on a fresh env: {0, 0, 10, 5.0, 40.0}.
 *  - pdrand_k in [0, 1): > 0, every control step draws its own gains per env and actuator u, kp_u ~ U((1 - k) kp[u], (1 + k) kp[u]) and
 *    kd_u likewise, and its frame_skip sub-steps run on them (robot_base.py:43-47).
 *  - sim_bemf != 0: every control step redraws, with probability 1 / bemf_interval (>= 1; the reference: 10), the env's back-EMF damping
 *    tau_d[u] ~ U(bemf_lo, bemf_hi) (0 <= bemf_lo <= bemf_hi, finite; the reference: 5, 40), and every sub-step applies
 *    tau = kp_u (q* - q) - kd_u w - tau_d[u] w (robot_base.py:53-60).  tau_d is per-env state: 0 at lhw_env_create, kept across
 *    lhw_env_reset and auto-resets (the reference's RobotBase outlives reset()), zeroed for every env by the call that turns sim_bemf off,
 *    kept by every other call.
 * Draws: lhw_rng.h on the STEP stream under the env's control-step counter (the one this step's task draws use), slots 128 + u (kp),
 * 144 + u (kd), 160 (back-EMF trigger), 161 + u (tau_d).  A reset runs no PD law and draws nothing.  With both off, every output is bit
 * for bit what it is without the feature: the kernels that carry it are a family of their own, launched only while one of the two is on.
 * That family exists for the launch-per-step calls (lhw_env_step / lhw_env_step_range) and the resident rollout of a feed-forward policy
 * without an observation history (lhw_env_rollout and its *_task_inputs forms), with and without the per-term statistics, on all four
 * humanoid tasks.  While it is on, lhw_env_rollout_lstm and lhw_env_rollout_history (history_len > 1) are declined with
 * LHW_ERR_UNSUPPORTED before anything is launched -- the caller steps the env launch by launch, as for any declined rollout -- and the
 * diagnostic clocks cannot be armed (see there).  HOST pointers; the setter synchronises the device (as lhw_env_set_state).  LHW_ERR_ARG,
 * with a message that names the field and nothing changed, for a value outside the ranges above; LHW_ERR_UNSUPPORTED for cartpole (its
 * robot class is not RobotBase). */
typedef struct {
  double pdrand_k;
  int32_t sim_bemf;
  int32_t bemf_interval;
  double bemf_lo, bemf_hi;
} LhwActuatorRand;
int lhw_env_set_actuator_randomization(LhwEnv* env, const LhwActuatorRand* settings);
int lhw_env_get_actuator_randomization(LhwEnv* env, LhwActuatorRand* out);
/* Parity hook: every env's back-EMF damping tau_d, HOST pointer [N][lhw_env_act_dim] float64, synchronous. */
int lhw_env_get_bemf_damping(LhwEnv* env, double* tau_d_host);
/* Task commands: which command an env of a fused walking or stepping task follows -- its mode and the speeds of that mode -- is decided
 * inside the control step by the reference's samplers, whose numbers are literals of tasks/walking_task.py:149-170, 194-205 and
 * tasks/stepping_task.py:261-334.  LhwTaskCommands holds them, batch-wide, from the next control step on, in every way a control step is
 * executed; a fresh env reports the reference's values, and with those every output is bit for bit what it is without the setter.
 * Walking tasks (jvrc_walk, h1_walk) read:
 *  - mode_cdf: the reset draw u in [0, 1) gives STANDING if u < [0], INPLACE if u < [1], else FORWARD (the reference: 0.6, 0.8).
 *    CUMULATIVE thresholds, stored and compared as given: get -> set changes no bit.
 *  - inplace_yaw, forward_vx, forward_vy: (lo, hi) of the uniform draws of the yaw rate (INPLACE: -0.5, 0.5), the forward speed (FORWARD:
 *    0, 0.4) and the lateral speed (FORWARD: 0, 0).  The draws keep their RNG slots; the lateral speed takes the third slot of the mode_ref
 *    draw, which FORWARD mode leaves free.  A range with lo == hi yields lo without a draw.  STANDING's three +-1 draws are not a setting.
 *  - switch_stand_every / switch_walk_every: every control step switches STANDING <-> INPLACE with odds 1 / n while both feet are in
 *    stance (100), and INPLACE <-> FORWARD with odds 1 / n (200).  0: that switch never fires and draws nothing.
 * The stepping task (jvrc_step) reads:
 *  - step_mode_cdf: u < [0] CURVED, < [1] STANDING, < [2] BACKWARD, < [3] LATERAL, else FORWARD (0.15, 0.2, 0.4, 0.7).
 *  - step_height_*: the stair height of FORWARD mode, clamp((iteration - start) / span, 0, 1) * max (3000, 8000, 0.1), with the
 *    iteration of lhw_env_set_iteration.  Its step length, gap and lateral width stay literals.
 * Each task reads its own group; the other group is validated and stored, and nobody reads it.
 * Pinned commands: per env, a mode (0 STANDING, 1 INPLACE, 2 FORWARD) and its mode_ref {yaw rate, forward speed, lateral speed} that the
 * kernels use for that env INSTEAD of drawing: at every task reset -- auto-resets inside a resident rollout included; the phase is still
 * drawn -- and at every task step, where a pinned env evaluates neither switch and takes mode and mode_ref from its pin before the reward
 * and the observation are formed, so a pin changed between two launches acts from the next control step on.  Mode -1 frees an env; free
 * envs, and every env before the first pin call, behave exactly as without the feature, also beside a pinned env in one wavefront.
 * lhw_env_pin_commands sets envs [first, first + count); lhw_env_get_pinned_commands reports the whole batch (-1 and zeros for a free env).
 * HOST pointers; all four calls synchronise the device (as lhw_env_set_task_shaping).  LHW_ERR_ARG, with a message that names the field and
 * nothing changed, for a non-finite value, a range with lo > hi, a cdf that does not ascend within [0, 1], a negative *_every,
 * step_height_span <= 0, a mode outside {-1, 0, 1, 2} or a pin range outside the batch.  LHW_ERR_UNSUPPORTED for cartpole and the h1
 * standing task (every call: they have no command), and for lhw_env_pin_commands on jvrc_step (its command is a footstep plan).  That
 * plan has a pin of its own: lhw_env_pin_step_plans / lhw_env_get_pinned_step_plans, below. */
typedef struct {
  double mode_cdf[2], inplace_yaw[2], forward_vx[2], forward_vy[2];
  int32_t switch_stand_every, switch_walk_every;
  double step_mode_cdf[4], step_height_start, step_height_span, step_height_max;
} LhwTaskCommands;
int lhw_env_set_task_commands(LhwEnv* env, const LhwTaskCommands* settings);
int lhw_env_get_task_commands(const LhwEnv* env, LhwTaskCommands* out);
int lhw_env_pin_commands(LhwEnv* env, int32_t first, int32_t count, const int32_t* mode_host /*[count], -1 frees*/,
                         const double* ref_host /*[count][3]*/);
int lhw_env_get_pinned_commands(LhwEnv* env, int32_t* mode_host /*[N]*/, double* ref_host /*[N][3]*/);
/* Pinned footstep plans: the stepping task's command is a walk mode and the footstep plan that goes with it, both drawn at every task
 * reset (tasks/stepping_task.py:278-311, 140-182).  An LhwStepPin replaces, for one env, the RESULT of the draws it names; every draw
 * keeps its RNG slot and counter and the phase is still drawn, so pinning exactly what an env would have drawn changes no bit.
 *  - mode: -1 frees the env (the other fields are then ignored and read back as zeros); else 0 CURVED, 1 STANDING, 2 BACKWARD,
 *    3 LATERAL, 4 FORWARD, the order of step_mode_cdf.  Besides selecting the generator it keeps its other meanings: the floor sinks
 *    under the stairs iff FORWARD, STANDING freezes the clocks and the goal update, LHW_TIN_MODE reports it.
 *  - choice: -1 leaves the mode's own draw alone.  CURVED: the row of the plan table, in [0, number of plans).  LATERAL: 0 walks to the
 *    side the draw 0 gives (sign -1), 1 to the other.  Every other mode: must be -1.
 *  - height: FORWARD: the signed rise per step, instead of the stair schedule's value (step_height_*) AND of the sign draw; NaN leaves
 *    both as they are.  Other modes do not read it.
 *  - nseq: 0: the sequence is generated from the mode.  2..20: steps[0 .. nseq) is the plan -- x, y, z, theta of each step relative to
 *    the feet mid-point and the root yaw at the reset, i.e. what generate_step_sequence returns -- and replaces the generated one.  The
 *    transform into the world frame, the fill of the unused rows, the targets and the terrain boxes follow from it as from a generated
 *    sequence.  steps beyond nseq are ignored and read back as zeros.
 *  - reserved: 0.
 * The pin acts at a task reset and nowhere else -- lhw_env_reset, every auto-reset of lhw_env_step / lhw_env_step_range, and the
 * auto-resets inside every resident rollout (lhw_env_rollout*, feed-forward, history and LSTM policies, with and without the term
 * statistics and the actuator randomisation) -- so it costs nothing per control step, and a pin changed between two launches acts from
 * the env's next reset on.  Free envs, and every env before the first call, behave exactly as without the feature, also beside a pinned
 * env.  lhw_env_pin_step_plans sets envs [first, first + count); lhw_env_get_pinned_step_plans reports the whole batch (mode -1 and zeros
 * for a free env; get -> set changes no bit).  HOST pointers; both calls synchronise the device.  LHW_ERR_ARG, with a message that names
 * the field and nothing changed, for a mode outside {-1 .. 4}, a choice outside its mode's range, nseq outside {0, 2 .. 20}, a
 * non-finite value among steps[0 .. nseq), an infinite height, reserved != 0 or a range outside the batch (an empty range at the end of
 * the batch lies inside it).  LHW_ERR_UNSUPPORTED for every env that is not jvrc_step. */
typedef struct { int32_t mode, choice, nseq, reserved; double height; double steps[20][4]; } LhwStepPin;
int lhw_env_pin_step_plans(LhwEnv* env, int32_t first, int32_t count, const LhwStepPin* pins_host /*[count]*/);
int lhw_env_get_pinned_step_plans(LhwEnv* env, LhwStepPin* out_host /*[N]; mode -1 and zeros for a free env*/);
/* Fault counters since the last call (host pointers, synchronous, resets them): control steps in which contacts were
 * dropped because more than the compiled-in cap were active (16 per env; the stepping task, whose feet rest on the floor AND on
 * the terrain boxes under them, merges identical contacts and holds 192 found / 64 distinct ones per sub-step), and control steps in which an env's state became
 * non-finite (the env is flagged terminated, its outputs are zeroed, and it is reset like any finished episode). */
int lhw_env_pop_fault_stats(LhwEnv* env, int64_t* contact_overflow, int64_t* diverged);
/* Control steps since the last call that the two-envs-per-wave kernels handed to the one-env-per-wave kernel because an
 * env touched more contacts than their layout holds (8); such a step costs roughly three ordinary ones.  Diagnostic of the
 * rollout, no reference counterpart (host pointer, synchronous, resets the counter). */
int lhw_env_pop_rerun_count(LhwEnv* env, int64_t* reruns);
/* Test / tuning hook for the update's GEMM kernel (no reference counterpart): C = op(A) op(B) on device buffers.
 * a_kc: A stored [M][K] (else [K][M]); b_kc: B stored [N][K] (else [K][N]); wt: 0 = automatic tile choice, 1 = 64x64, 2 = 128x128
 * block tiles, 16 = fp16 operands (64x64 tiles, fp16 MFMA); optional epilogue bias[n], ReLU, mask (v = mask[m][n] > 0 ? v : 0).
 * With `part` (split-K scratch,
 * [ceil(K / k_chunk)][M*N] floats) the partial products are reduced in slice order and ADDED to C, as the weight-gradient GEMMs
 * of lhw_ppo_grad do; `colsum` ([slices][M] scratch, A stored [K][M] only) also ADDS sum_k A[k][m] to colsum_out[m] (the bias
 * gradient fused into the same pass).  Leading dimensions must be multiples of 4 floats (16-byte rows). */
int lhw_debug_gemm(int32_t a_kc, int32_t b_kc, int32_t wt, int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B,
                   int32_t ldb, float* C, int32_t ldc, const float* bias, int32_t relu, const float* mask, int32_t ldmask,
                   int32_t k_chunk, float* part, float* colsum, float* colsum_out, void* stream);
/* Test hook for the wide weight gradient of the update (csrc/lhw_gemm.hip: wgrad_wide_kernel; reference /root/reference/rl/algos/ppo.py:387-396,
 * the hidden layer's part of loss.backward()): per k slice z of k_chunk rows, part[z] [256][256] = A[rows of z]^T B[rows of z] and
 * colsum[z] [256] = column sums of A's rows (A, B: [K][256] device buffers, dh2 and h1; colsum may be NULL).  The caller reduces the slices. */
int lhw_debug_wgrad_wide(const float* A, const float* B, int32_t K, int32_t k_chunk, float* part, float* colsum, void* stream);
/* Test hook for the fused skinny weight gradients of the update (csrc/lhw_gemm.hip: wgrad_skinny_kernel; reference
 * /root/reference/rl/algos/ppo.py:387-396, the first- and last-layer parts of loss.backward()): dW1 [H][Dp] += dh1^T x, db1 += colsum(dh1),
 * dW3 [O][H] += dy^T h2, db3 += colsum(dy) over R rows in one launch.  H = 256, Dp <= 64 (multiple of 4), O <= Op <= 32; device buffers;
 * scratch: ceil(R / max(128, ceil(R / 256))) x (256 Dp + 256 + 256 O + O) floats. */
int lhw_debug_wgrad_skinny(int32_t H, int32_t Dp, int32_t O, int32_t Op, const float* dh1, const float* x, int32_t ldx, const float* dy,
                           const float* h2, int32_t R, float* dW1, float* db1, float* dW3, float* db3, float* scratch, void* stream);
/* Test hooks for the LDS-resident strip kernels of the update's MLPs (csrc/lhw_mlp_strip.hip; reference:
 * /root/reference/rl/algos/ppo.py:299-406, the actor / critic forward and the activation gradients of loss.backward()):
 * forward  h1 = relu(x W1^T + b1), h2 = relu(h1 W2^T + b2), y = h2 W3^T + b3 for R rows in one launch;
 * backward dh2 = (dy W3) * (h2 > 0), dh1 = (dh2 W2) * (h1 > 0).  Weights in torch Linear layout ([out][in]; W1 row stride Dp,
 * a multiple of 4; W3 [Op][H]); device buffers; H must be 256, Dp <= LHW_MLP_STRIP_MAX_IN_PAD, O <= 32 (LHW_ERR_UNSUPPORTED otherwise, with
 * nothing written).  Dp <= 64: the read-out y is the ascending sum of eight 32-k partial chains; Dp > 64 (the wide instantiations): ONE chain over
 * k with the bias behind it, bitwise the per-layer GEMMs and lhw_debug_policy_step's plain launch.  wt_scratch: (Dp + 256 + Op) * 256 floats for
 * the transposed weight copies the forward kernel reads. */
int lhw_debug_mlp_strip_forward(int32_t H, int32_t Dp, int32_t O, int32_t Op, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, const float* x, int32_t ldx, int32_t R,
                                float* h1, float* h2, float* y, float* wt_scratch, void* stream);
int lhw_debug_mlp_strip_backward(int32_t H, int32_t O, int32_t Op, const float* w2, const float* w3, const float* dy, int32_t R,
                                 const float* h1, const float* h2, float* dh2, float* dh1, void* stream);
/* The same two launches with the ReLU masks handed over as BITS (round 6): the forward launch also writes, per hidden layer,
 * ceil(R / 64) * 512 words (bit set = activation positive, in the kernels' own thread-to-element order); a backward launch over the same
 * R rows given those words does not read h1 / h2 (which may then be NULL).  64-row slabs whatever the row count. */
int lhw_debug_mlp_strip_forward_bits(int32_t H, int32_t Dp, int32_t O, int32_t Op, const float* w1, const float* b1, const float* w2,
                                     const float* b2, const float* w3, const float* b3, const float* x, int32_t ldx, int32_t R, float* h1,
                                     float* h2, float* y, float* wt_scratch, uint32_t* bits1, uint32_t* bits2, void* stream);
int lhw_debug_mlp_strip_backward_bits(int32_t H, int32_t O, int32_t Op, const float* w2, const float* w3, const float* dy, int32_t R,
                                      const float* h1, const float* h2, float* dh2, float* dh1, const uint32_t* bits1, const uint32_t* bits2,
                                      void* stream);
/* Test hooks for the fp16 strip kernels (csrc/lhw_mlp_strip_h.hip; the --fp16 update and fp16 inference behind lhw_ppo_debug_set_strip_fp16): the
 * same two passes with fp16 operands on v_mfma_f32_32x32x16_f16, float32 accumulation, the activations between the layers in LDS as fp16 -- bit
 * for bit three / two lhw_debug_gemm launches in the fp16-operand, fp16-storage modes (wt = 16 + bits).  Weights float32 in torch Linear layout;
 * the entry makes the kernels' fp16 copies of them in wh_scratch (163840 halves, 16-byte aligned) first.  forward: x is float32 [R][ldx] (x_half = 0: rounded while staged) or fp16 [R][ldx] (x_half != 0; ldx counts halves);
 * h1_h / h2_h fp16 [R][256], written once (both may be NULL: they never leave LDS); y float32 [R][Op], columns < O written.  backward: dy float32
 * [R][Op]; h1_h / h2_h the stored fp16 activations (the masks, > 0); dh2_h / dh1_h fp16 [R][256].  fp16 buffers 16-byte aligned.
 * Shapes: H = 256, Dp <= 64 (a multiple of 4), O <= 32, Op >= O; others return LHW_ERR_UNSUPPORTED with nothing written. */
int lhw_debug_mlp_strip_forward_h(int32_t H, int32_t Dp, int32_t O, int32_t Op, const float* w1, const float* b1, const float* w2,
                                  const float* b2, const float* w3, const float* b3, const void* x, int32_t ldx, int32_t x_half, int32_t R,
                                  void* h1_h, void* h2_h, float* y, void* wh_scratch, void* stream);
int lhw_debug_mlp_strip_backward_h(int32_t H, int32_t O, int32_t Op, const float* w2, const float* w3, const float* dy, int32_t R,
                                   const void* h1_h, const void* h2_h, void* dh2_h, void* dh1_h, void* wh_scratch, void* stream);
/* Test hook for the update's train strip kernel (csrc/lhw_mlp_strip.hip: forward layers, PPO head, backward layers of one network on slabs
 * that stay in LDS): one network's pass over a minibatch of B rows.  critic = 0: the actor (O = act_dim outputs in rows of Op <= 64; act [B][O],
 * old_logp / adv [B], stdv [O]); twin0 > 0 adds the mirror term: rows [twin0, twin0 + B) of x / h1 / h2 / y / dy / dh2 / dh1 are the mirrored
 * twins of rows [0, B) (twin0 >= B; act_src / act_sign [O]).  critic = 1: the value head (O = 1, Op = 4; ret [B]).  Outputs, device buffers:
 * h1 / h2 / dh2 / dh1 [rows][256], y / dy [rows][Op], dstd [B][Op] (actor, nullable), stat_rows [6][stat_ld]: every row's terms of the loss
 * scalars in lhw_ppo_grad's order (the actor writes all but term 1, the critic term 1).  fused = 1: one launch.  fused = 0: the forward
 * strip, the head as a thread-per-row kernel on y in HBM, the backward strip -- the same arithmetic, bit for bit.  Dp in (64,
 * LHW_MLP_STRIP_MAX_IN_PAD] (the wide instantiation): fused = 0 is instead the per-layer GEMM path that launch takes over, in independent code --
 * a plain thread-per-output fmaf chain per layer with the GEMM's bias / ReLU / mask epilogue around the same head kernel; bit for bit again. */
typedef struct LhwTrainStripArgs {
  int32_t H, Dp, O, Op;
  const float *w1, *b1, *w2, *b2, *w3, *b3;   /* torch Linear layout, as lhw_debug_mlp_strip_forward */
  const float* x;
  int32_t ldx, B, twin0, critic;
  const float *act, *old_logp, *adv, *ret, *stdv;
  float clip, mirror_coeff;
  const int32_t* act_src;
  const float* act_sign;
  float *h1, *h2, *y, *dy, *dh2, *dh1, *dstd, *stat_rows;
  int32_t stat_ld;
  float* wt_scratch;                          /* (Dp + 256 + Op) * 256 floats */
} LhwTrainStripArgs;
int lhw_debug_mlp_train_strip(const LhwTrainStripArgs* args, int32_t fused, void* stream);
/* Test hook: the rollout's per-control-step policy launch (observation normalisation -> actor -> Gaussian head, one strip launch;
 * what lhw_ppo_forward_at runs when only act / logp are requested) on R raw observation rows [R][obs_dim], from an actor view.
 * y [R][act_pad] receives the means.  The reference of lhw_env_rollout's in-wave policy step (bitwise).  obs_pad in (64,
 * LHW_ROLLOUT_HISTORY_MAX_OBS_PAD] (an observation history): a plain launch, a workgroup per row and a thread per hidden unit, in the
 * order of the per-layer GEMM forward -- the reference of lhw_env_rollout_history's in-wave step (bitwise) at every width it accepts. */
int lhw_debug_policy_step(const LhwRolloutPolicy* policy, const float* obs, int32_t R, uint32_t env_id_base, uint32_t counter, float* y,
                          float* act, float* logp, void* stream);
/* Test hook: lhw_rnn_forward's actor step (normalisation -> two LSTM cells -> read-out -> Gaussian head, commit = 1) on R raw observation
 * rows [R][obs_dim] as ONE plain launch from an LSTM actor view -- a thread per hidden unit, the fmaf chains and the cell function of the
 * in-wave step.  reset [R] u8 (nullable): rows that start an episode.  Advances rows 0 .. R - 1 of the view's state; y [R][act_pad] receives
 * the means.  The per-step reference of lhw_env_rollout_lstm where lhw_rnn_forward is not built (SIMT emulator); bitwise equal to both. */
int lhw_debug_lstm_policy_step(const LhwRolloutLstmPolicy* policy, const float* obs, int32_t R, const uint8_t* reset, uint32_t env_id_base,
                               uint32_t counter, float* y, float* act, float* logp, void* stream);
/* Test hook for the recurrent update's whole-sequence strip kernels (csrc/lhw_mlp_strip.hip: lstm_seq_fwd_strip_kernel /
 * lstm_seq_bwd_strip_kernel; the time loops of lhw_rnn_grad, reference rl/algos/ppo.py:512-533 over Gaussian_LSTM_Actor / LSTM_V,
 * rl/policies/actor.py:191-286, critic.py:52-112): the forward pass and the BPTT of ONE network's two stacked cells over a [T][Bt] sequence
 * minibatch (rows r = t * Bt + b) on caller-owned device buffers, without the read-out, the loss and the weight gradients.  w1 [4H][Dp + H] =
 * [W_ih1 | W_hh1], w2 [4H][2H] = [W_ih2 | W_hh2], biases [4H] (gate order i f g o); reset [T][Bt] u8: an episode starts at step t of row b.
 * passes & 1, forward: reads the x columns of xh1 [R][Dp + H]; writes its recurrent columns, xh2 [R][2H], the activated gates g1 / g2 [R][4H],
 * c1 / c2 / h2 [R][H].  passes & 2, backward: reads those and dh2 [R][H] (d loss / d h2) and overwrites g1 / g2 with d loss / d pre-activation.
 * scratch: (Dp + 3H) * 4H + 5 * Bt * H floats.  fused = 1: one launch per pass (LHW_ERR_UNSUPPORTED outside the LHW_LSTM_SEQ_* bounds; every
 * buffer 16-byte aligned).  fused = 0: the launch-per-step loops with a thread-per-output fmaf-chain kernel for the products and the two
 * functions of csrc/lhw_lstm_cell.h -- any shape, the same arithmetic, bit for bit. */
typedef struct LhwLstmSeqArgs {
  int32_t H, Dp, T, Bt, passes;
  const float *w1, *bi1, *bh1, *w2, *bi2, *bh2;
  const uint8_t* reset;
  const float* dh2;
  float *xh1, *xh2, *g1, *g2, *c1, *c2, *h2;
  float* scratch;
} LhwLstmSeqArgs;
int lhw_debug_lstm_seq(const LhwLstmSeqArgs* args, int32_t fused, void* stream);
/* Test hook for lhw_rnn_values' kernel (csrc/lhw_mlp_strip.hip: lstm_seq_value_strip_kernel): ONE network of two stacked cells and a read-out of
 * one output over a stored rollout of N env rows, on caller-owned device buffers.  Weights as in LhwLstmSeqArgs, wo [H], bo [1]; obs [T + 1][N][D]
 * and term_obs [T][N][D] RAW observations, obs_mean / obs_std [D]; done [T][N], reset0 [N] (nullable).  The state is kept the way the handle keeps
 * it: in the recurrent columns of xh1 [N][Dp + H] = [x | h1] and xh2 [N][2H] = [h1 | h2] and in c1 / c2 [N][H]; it is read and left advanced by T
 * steps.  val [T][N]; vterm [T][N] with term_obs (both or neither); vfinal [N] nullable.  scratch: max((Dp + 3H) * 4H, 6 N H) floats.
 * fused = 1: one launch (LHW_ERR_UNSUPPORTED outside the LHW_LSTM_SEQ_* bounds; c1 / c2 16-byte aligned); the other columns of xh1 / xh2 are not
 * touched.  fused = 0: per time slice the launches of lhw_rnn_forward's step with a thread-per-output fmaf-chain kernel for the products -- any
 * shape, the same arithmetic, bit for bit. */
typedef struct LhwLstmValuesArgs {
  int32_t H, D, Dp, T, N;
  const float *w1, *bi1, *bh1, *w2, *bi2, *bh2, *wo, *bo;
  const float *obs_mean, *obs_std;
  const float *obs, *term_obs;
  const uint8_t *done, *reset0;
  float *xh1, *xh2, *c1, *c2;
  float *val, *vterm, *vfinal;
  float* scratch;
} LhwLstmValuesArgs;
int lhw_debug_lstm_values(const LhwLstmValuesArgs* args, int32_t fused, void* stream);
/* The two diagnostic clocks of the humanoid steppers, lhw_env_debug_wave_cycles (wave clock) and lhw_env_phase_cycles (phase clock).
 * The kernels the product runs carry neither clock.  Once a clock of an env is armed (it stays armed for the env's life), the env's control
 * steps run a second set of kernels that do: every launch-per-step control step (lhw_env_step / lhw_env_step_range, all tasks) and the
 * resident rollout of a feed-forward policy without an observation history (lhw_env_rollout and its *_task_inputs forms, all tasks, the
 * job queue of the stepping task included).  Every value a step stores is the same, bit for bit, with and without the clocks.
 * What has no kernels with clocks never runs with a clock armed, so that no call records nothing without saying so:
 *  - lhw_env_rollout_lstm and lhw_env_rollout_history on an env with an armed clock fail with LHW_ERR_UNSUPPORTED before anything is
 *    launched -- the code with which a resident rollout is declined for any other reason; the caller steps the env launch by launch
 *    (BatchedEnv.rollout returns False), and those steps record.
 *  - The clocks and the per-term episode statistics exclude each other: arming a clock while lhw_env_enable_term_stats is in force, and
 *    lhw_env_enable_term_stats(env, 1) on an env with an armed clock, fail with LHW_ERR_UNSUPPORTED and change nothing.
 *  - Likewise the clocks and the actuator randomisation: arming a clock while pdrand_k > 0 or sim_bemf is set, and a
 *    lhw_env_set_actuator_randomization that sets either on an env with an armed clock, fail with LHW_ERR_UNSUPPORTED and change nothing. */
/* Diagnostic (load balance): the first call arms the recording; later calls return, per env, the shader-clock cycles its
 * wavefront group spent in the most recent control-step launch (after a resident rollout: in all control steps of the rollout).
 * HOST pointer [N] int64, synchronous; humanoid tasks only. */
int lhw_env_debug_wave_cycles(LhwEnv* env, int64_t* cycles_host);
int lhw_env_set_iteration(LhwEnv* env, int64_t iteration);
/* Diagnostic: shader-clock cycles env 0 spent in each phase of the wave-per-env stepper since the last call
 * (slots: 0 kinematics, 1 com/cdof, 2 CRBA, 3 collision, 4 constraint rows, 5 velocity/RNE, 6 smooth solve,
 * 7 Newton, 8 Euler tail (integration), 9 whole control step incl. the above, 10 task/reward/reset,
 * 11 actuation + row loads + reference acceleration, 12 factor/solve of M, 13 factor/solve of M + h*damping).
 * enable != 0 turns the counters on. */
int lhw_env_phase_cycles(LhwEnv* env, int enable, int64_t* out16);
/* Diagnostic: resident workgroups per CU the HIP runtime reports for the wave-per-env step kernel. */
int lhw_debug_stepper_occupancy(void);
/* Test hook: the cross-lane (DPP) fetches of the humanoid steppers in their two forms -- the reference form, which passes the identity of a
 * lane without a source as the `old` operand, and the form the kernels run, which takes a zero identity word from bound_ctrl (csrc/
 * lhw_humanoid_dev.h: dpp_d_ref / dpp_d, rbc_ref / rbc, gscan_lanes).  ONE wavefront; lane l takes part iff bit l of lane_mask is set, reads
 * in[l] (DEVICE pointer, [64] doubles) and stores what it fetched, as bits, to out_ref / out_shipped [LHW_DPP_FORMS][64] (device): rows 0-3
 * row_shr 1 2 4 8 and rows 4-7 row_shl 1 2 4 8 with identity 0.0, row 8 row_shr:1 with identity 1.0, row 9 with +inf, rows 10-13
 * row_newbcast of row positions 0 2 5 15, rows 14 / 15 the inclusive int scan of ((low ^ high word) & 0xffff) with one env / two envs per
 * wave, its masked row_bcast steps included.  Entries of lanes outside the mask are left as the caller filled them.  The two outputs are
 * equal bit for bit, except that a row_newbcast whose source lane is outside the mask returns the lane's own value in the reference form and
 * 0 in the other (no kernel reads either). */
#define LHW_DPP_FORMS 16
int lhw_debug_dpp_forms(uint64_t lane_mask, const double* in, uint64_t* out_ref, uint64_t* out_shipped, void* stream);
/* Test hook: the fp64 helpers the humanoid steppers use in place of IEEE `/` and sqrt() (csrc/lhw_humanoid_dev.h: the v_rcp_f64 / v_rsq_f64
 * seed plus two Newton steps), one launch over n input pairs, 1 <= n <= 2^24.  DEVICE pointers, [n] doubles each: out_rcp[i] = rcp_f64(b[i]),
 * out_qdiv[i] = qdiv(a[i], b[i]), out_rsqrt[i] = rsqrt_f64(b[i]), out_qsqrt[i] = qsqrt(b[i]).  Not IEEE at the ends: a zero or infinite
 * b gives NaN from the first three, a negative or infinite b gives NaN from the roots, qsqrt(+-0) is +0. */
int lhw_debug_fastmath(int64_t n, const double* a, const double* b, double* out_rcp, double* out_qdiv, double* out_rsqrt, double* out_qsqrt,
                       void* stream);

/* ------------------------------------------------------------------ PPO (actor/critic MLP, GAE, update) */
typedef struct LhwPpo LhwPpo;

typedef struct {
  int32_t device;
  int32_t obs_dim, act_dim, hidden; /* reference networks: 2 x 256 ReLU (rl/policies/actor.py:127) */
  int32_t learn_std;                /* --learn-std: stds are a parameter (actor.py:145-148) */
  int32_t max_rows;                 /* workspace capacity: max rows per forward / minibatch */
  float lr, eps;                    /* Adam lr and eps; eps is also the advantage-normalisation eps (ppo.py:429-430,485) */
  float clip, entropy_coeff, mirror_coeff, max_grad_norm;
  /* signed-permutation mirror tables (NULL = no mirror loss): out[j] = sign[j] * in[src[j]]
   * == x @ _get_symmetry_matrix(...) with the clock sign flip folded in (rl/envs/wrappers.py:53-85) */
  const int32_t* mirror_obs_src; const float* mirror_obs_sign; /* [obs_dim] */
  const int32_t* mirror_act_src; const float* mirror_act_sign; /* [act_dim] */
} LhwPpoConfig;

int lhw_ppo_create(const LhwPpoConfig* cfg, LhwPpo** out);
int lhw_ppo_destroy(LhwPpo* ppo);
/* number of float32 in the flat parameter vector theta (actor | stds | critic, internally padded) */
int64_t lhw_ppo_param_count(const LhwPpo* ppo);
/* offsets of actor W1,b1,W2,b2,W3,b3, stds, critic W1..b3, then padded obs width and padded actor out width */
int lhw_ppo_layout(const LhwPpo* ppo, int64_t* out15);
/* xn (and xm if non-NULL) [R][pad4(obs_dim)] <- (obs - mean)/std of R raw rows (mirrored for xm) */
int lhw_ppo_normalize(LhwPpo* ppo, const float* obs, int64_t R, const float* obs_mean, const float* obs_std, float* xn,
                      float* xm, void* stream);
/* rollout inference on N rows: mu/act/logp [N][act_dim]/[N][act_dim]/[N], value [N]; any output group may be NULL */
int lhw_ppo_forward(LhwPpo* ppo, const float* theta, const float* obs, int64_t N, const float* obs_mean,
                    const float* obs_std, uint64_t seed, uint32_t env_id_base, uint32_t counter, int deterministic,
                    float* mu, float* act, float* logp, float* value, void* stream);
/* Rollout bracket.  theta does not change while a rollout is collected (the reference's workers hold a frozen copy of the policy,
 * rl/workers/rollout_worker.py:62-77 sync_policy), so the [in][out] weight copies the forward strip kernel multiplies by are made
 * ONCE here (on `stream`; streams that issue forwards afterwards must be ordered behind it) instead of in every policy step.
 * Until lhw_ppo_end_rollout -- or lhw_ppo_apply, which changes theta -- every lhw_ppo_forward / _forward_at call with this theta
 * pointer reads those copies (read-only: any number of concurrent calls on any streams).  Outside a bracket each call makes
 * its own copies, as before.  theta must NOT be written between lhw_ppo_begin_rollout and lhw_ppo_end_rollout (a checkpoint load, a
 * parameter broadcast): the bracket is keyed by the pointer, so the copies would silently go stale -- close it first (the Python
 * layer's PpoKernels.set_tensors does). */
int lhw_ppo_begin_rollout(LhwPpo* ppo, const float* theta, void* stream);
int lhw_ppo_end_rollout(LhwPpo* ppo);
/* Inside a rollout bracket opened with this theta: the actor of theta as lhw_env_rollout reads it (the bracket's [in][out]
 * weight copies, biases and stds inside theta, the caller's normalisation vectors).  Valid until lhw_ppo_end_rollout /
 * lhw_ppo_apply.  LHW_ERR_UNSUPPORTED outside a bracket or for shapes the in-wave steps do not cover (hidden width 256; padded observation
 * width <= 64, or <= LHW_ROLLOUT_HISTORY_MAX_OBS_PAD for lhw_env_rollout_history).  With fp16 inference selected
 * (lhw_ppo_set_inference_dtype) the view asks for fp16 operands: the in-wave policy step then rounds weights and activations to fp16 and
 * accumulates in float32 over ascending k -- the fp16 MFMA of the launch-per-step path adds its 16 products per instruction in its own
 * order, so in THAT mode the two rollouts agree to float32 rounding (1e-6), not bitwise. */
int lhw_ppo_rollout_policy(LhwPpo* ppo, const float* theta, const float* obs_mean, const float* obs_std, uint64_t seed,
                           uint32_t counter, int deterministic, LhwRolloutPolicy* out);
/* lhw_ppo_forward on workspace rows [ws_row, ws_row + N): calls issued on different streams for disjoint env groups may run
 * concurrently (env_id_base must be the global id of the group's first env) */
int lhw_ppo_forward_at(LhwPpo* ppo, const float* theta, const float* obs, int64_t N, const float* obs_mean,
                       const float* obs_std, uint64_t seed, uint32_t env_id_base, uint32_t counter, int deterministic,
                       int64_t ws_row, float* mu, float* act, float* logp, float* value, void* stream);
/* fp16 != 0: lhw_ppo_forward (rollout inference) rounds weights and activations to fp16 and multiplies on the fp16 MFMA with
 * float32 accumulation (BASELINE config "fp16 actor/critic"); the update (lhw_ppo_grad) uses float32 operands unless
 * lhw_ppo_set_update_dtype selects fp16 as well */
int lhw_ppo_set_inference_dtype(LhwPpo* ppo, int fp16);
/* fp16 != 0: every GEMM of lhw_ppo_grad (forward, activation gradients, weight gradients) rounds both operands to fp16 and
 * runs on the fp16 MFMA with float32 accumulation -- BASELINE config 5 "fp16 actor/critic": fp16 weights and activations per
 * GEMM, float32 master weights, loss, gradient accumulation and Adam.  The reference has no counterpart (it trains in float32). */
int lhw_ppo_set_update_dtype(LhwPpo* ppo, int fp16);
/* debug / A-B: on != 0: lhw_ppo_grad runs each network's forward, loss head and backward layers as ONE train strip launch where it can
 * (float32 update, no armed imitation term, hidden width 256); 0: forward strip, ppo_loss_kernel, backward strip.  Same bits either way.
 * A new handle takes the environment's LHW_STRIP_FUSED (default 1). */
int lhw_ppo_debug_set_strip_fused(LhwPpo* ppo, int32_t on);
/* debug / A-B: networks whose padded observation row is wider than 64 columns (an observation history; up to LHW_MLP_STRIP_MAX_IN_PAD).  on != 0:
 * wherever the handle chooses between a strip launch and per-layer GEMMs -- rollout inference, the critic's values behind the resident rollout,
 * the one-launch policy step of lhw_ppo_forward_at, lhw_ppo_grad's forward / backward strips and train strips -- such shapes take the wide strip
 * instantiations, under the conditions that hold for narrow shapes (float32; no armed imitation term for the train strips).  0 (a new handle):
 * they run one GEMM per layer.  Same bits either way: the wide strips compute the GEMM path's chains.  The skinny weight gradients of such
 * shapes stay split-K GEMMs.  Closes an open rollout bracket (lhw_ppo_begin_rollout makes the critic's weight copies for the path chosen). */
int lhw_ppo_debug_set_strip_wide(LhwPpo* ppo, int32_t on);
/* debug / A-B: the fp16 strip kernels (csrc/lhw_mlp_strip_h.hip) for narrow shapes (hidden 256, padded observation row <= 64 columns).  on != 0:
 * a --fp16 update with fp16 storage (lhw_ppo_set_update_dtype; not LHW_FP16_STORAGE=0) runs each network's forward layers as one forward strip
 * launch and its activation gradients as one backward strip launch (LHW_MLP_STRIP >= 1; the plan reports fwd_strip = bwd_strip = 3, no train
 * strips, no mask bits; the weight gradients stay split-K fp16 GEMMs), and fp16 inference (lhw_ppo_set_inference_dtype) runs the forward strip in
 * lhw_ppo_forward[_at] (LHW_MLP_STRIP >= 2; infer_strips = 1; the one-launch policy step stays float32-only).  0 (a new handle): one fp16 GEMM per
 * layer.  Same bits either way: the strips compute the GEMM path's chains on the same MFMA.  The first call with on != 0 allocates the kernels'
 * fp16 weight copies (6.5 MB; LHW_ERR_HIP if that fails, the handle unchanged); every call closes an open rollout bracket.  The Python layer
 * passes LHW_STRIP_FP16 on. */
int lhw_ppo_debug_set_strip_fp16(LhwPpo* ppo, int32_t on);
/* test hook: 1 if the last lhw_ppo_grad of this handle (a captured one included) ran the train strip launches, 0 if the three-launch path */
int lhw_ppo_debug_last_grad_fused(const LhwPpo* ppo);
/* test hook: which kernels the handle's calls launch, as the handle itself decides it -- once per call, from its switches (read from the LHW_*
 * environment when it was created; the three debug setters above), the update dtype, the network shape and the row capacity.
 * out13[0..8): the plan of an lhw_ppo_grad call on a minibatch of B rows (imitation != 0: with an imitation term armed) -- fp16 operands,
 * fp16 storage, forward strips, backward strips (masks: 1 actor | 2 critic), train strips, mask bits, wide instantiations, streams (1 | 2).
 * out13[8..13): lhw_ppo_forward[_at] and the rollout bracket -- fp16 operands, forward launches run the strips, the one-launch policy step is
 * available, lhw_ppo_begin_rollout makes the critic's weight copies, ... the actor's (the bracket opens). */
int lhw_ppo_debug_plan(const LhwPpo* ppo, int32_t B, int32_t imitation, int32_t* out13);
/* time-major [T][N] GAE(lambda); done holds LHW_DONE_* flags, vterm the critic value of the terminal
 * observation, vfinal [N] the value of the observation after the last step */
int lhw_gae(int32_t T, int32_t N, const float* rew, const float* val, const uint8_t* done, const float* vterm,
            const float* vfinal, double gamma, double lam, float* ret, float* adv, void* stream);
int lhw_moments(const float* x, int64_t n, double* out2_dev, void* stream);
int lhw_scale_shift(float* x, int64_t n, float mean, float inv_scale, void* stream);
/* x <- (x - mean) / (std + eps), mean and UNBIASED std taken on the device from stats3_dev = {sum, sum of squares, count} (float64;
 * e.g. lhw_moments' output with the count appended, summed over ranks by an all-reduce): the advantage normalisation of
 * rl/algos/ppo.py:484-485 over the global batch without a device -> host round trip */
int lhw_standardize(float* x, int64_t n, const double* stats3_dev, double eps, void* stream);
/* Imitation term of the NEXT lhw_ppo_grad call (reference rl/algos/ppo.py:360-368, rl/algos/imitation.py): the host
 * evaluates env.imitation_projector() and the frozen expert policy, and passes the expert means scattered into a dense
 * [B][act_dim] target with a [B][act_dim] 0/1 mask (minibatch row order), the coefficient and the number of selected
 * entries (denominator of the mean).  NULL target disarms. */
int lhw_ppo_set_imitation(LhwPpo* ppo, const float* target, const uint8_t* mask, float coeff, int64_t n_selected);
/* forward + loss + backward of one minibatch; accumulates into grad and stats_dev[0..5]
 * (actor, critic, mirror, approx_kl, clip_fraction, imitation) */
int lhw_ppo_grad(LhwPpo* ppo, const float* theta, float* grad, const float* xn, const float* xm, const float* act,
                 const float* old_logp, const float* adv, const float* ret, const int32_t* idx, int32_t B,
                 float* stats_dev, void* stream);
/* dual clip_grad_norm_ + Adam; zeroes grad */
int lhw_ppo_apply(LhwPpo* ppo, float* theta, float* grad, float* adam_m, float* adam_v, int64_t step, float grad_scale,
                  void* stream);
/* test hook: synchronises the device and copies to the host the two squared gradient norms (actor group, critic group; the gradient
 * times grad_scale, before clipping) that the last lhw_ppo_apply / lhw_ppo_step clipped with */
int lhw_ppo_debug_grad_sqnorms(LhwPpo* ppo, float* out2_host);
/* lhw_ppo_grad followed by lhw_ppo_apply as ONE launch: the optimiser step of rl/algos/ppo.py:387-396 (zero_grad, backward, two
 * clip_grad_norm_, two Adam steps) captured once as a hipGraph per (buffers, minibatch size, grad_scale) and replayed, the minibatch's
 * index pointer and Adam's bias corrections patched into the graph's kernel nodes (a new grad_scale recaptures).  Bitwise the result of
 * the two calls.  Single process only: with data
 * parallelism the gradient all-reduce belongs between lhw_ppo_grad and lhw_ppo_apply. */
int lhw_ppo_step(LhwPpo* ppo, float* theta, float* grad, float* adam_m, float* adam_v, const float* xn, const float* xm, const float* act,
                 const float* old_logp, const float* adv, const float* ret, const int32_t* idx, int32_t B, float* stats_dev, int64_t step,
                 float grad_scale, void* stream);

/* ------------------------------------------------------------------ recurrent PPO (LSTM actor / critic)
 * Gaussian_LSTM_Actor / LSTM_V: two stacked LSTMCells (hidden) + linear read-out (reference rl/policies/actor.py:191-286,
 * critic.py:52-112); rollout one cell step per control step with state reset at episode starts
 * (rl/workers/rollout_worker.py:134-137,174-177); update by BPTT over whole trajectories (rl/algos/ppo.py:512-533) --
 * a minibatch is a set of env columns of the time-major rollout, with the state zeroed where an episode starts inside a
 * column (equivalent to the reference's padded trajectory list with masked losses).  Uses LhwPpoConfig (max_rows unused). */
typedef struct LhwRnn LhwRnn;
int lhw_rnn_create(const LhwPpoConfig* cfg, int32_t seq_len, int32_t seq_cols, int32_t rollout_rows, LhwRnn** out);
int lhw_rnn_destroy(LhwRnn* rnn);
int64_t lhw_rnn_param_count(const LhwRnn* rnn);
/* offsets: [0..7] actor Wcat1 ([4H][pad4(obs)+H] = [W_ih | W_hh]) b_ih1 b_hh1 Wcat2 ([4H][2H]) b_ih2 b_hh2 Wout bout,
 * [8] stds, [9..16] critic likewise, [17] padded obs width, [18] padded actor read-out width */
int lhw_rnn_layout(const LhwRnn* rnn, int64_t* out19);
/* one rollout step on N rows; reset [N] (device, may be NULL) marks rows whose episode starts with this observation;
 * commit != 0 advances the stored hidden state, 0 evaluates only (terminal / final values) */
int lhw_rnn_forward(LhwRnn* rnn, const float* theta, const float* obs, int64_t N, const float* obs_mean, const float* obs_std,
                    const uint8_t* reset, uint64_t seed, uint32_t env_id_base, uint32_t counter, int deterministic, int commit,
                    float* mu, float* act, float* logp, float* value, void* stream);
/* The critic of theta over a stored rollout: bitwise the values and the critic state that
 *   for t in 0..T-1: lhw_rnn_forward(obs[t], reset = t ? done[t-1] != 0 : reset0, commit = 1, value = val[t]);
 *                    lhw_rnn_forward(term_obs[t], commit = 0, value = vterm[t]);
 *   lhw_rnn_forward(obs[T], commit = 0, value = vfinal)
 * leave behind, in ONE launch (plus the [in][out] copies of the critic's two weight matrices, made on `stream`); the actor's state is not touched.
 * obs [T + 1][N][obs_dim], term_obs [T][N][obs_dim] raw observations; done [T][N] LHW_DONE_* flags; reset0 [N] (nullable).  term_obs / vterm
 * nullable (together), vfinal nullable.  N <= rollout_rows.  term_obs[t] must equal obs[t + 1] on every row whose done[t] is 0 -- what
 * lhw_env_step / lhw_env_rollout* write -- : where no row of a 32-row slab ended an episode at step t, vterm[t] is taken from val[t + 1].
 * LHW_ERR_UNSUPPORTED, with nothing written, outside the LHW_LSTM_SEQ_* bounds below: the caller keeps the per-step calls. */
int lhw_rnn_values(LhwRnn* rnn, const float* theta, const float* obs, const float* term_obs, const uint8_t* done,
                   const uint8_t* reset0, int32_t T, int32_t N, const float* obs_mean, const float* obs_std,
                   float* val, float* vterm, float* vfinal, void* stream);
/* The actor of theta as lhw_env_rollout_lstm reads it: makes the [in][out] copies of the three weight matrices on `stream` (theta is
 * frozen during a rollout: rl/workers/rollout_worker.py:62-77 sync_policy) and fills the view with them, the biases and stds inside
 * theta, the caller's normalisation vectors and the handle's own actor state buffers.  Valid until the next lhw_rnn_apply (or any other
 * write to theta) or lhw_rnn_destroy.  LHW_ERR_UNSUPPORTED for hidden != 256 or shapes the in-wave lane mapping does not cover
 * (padded observation width > 64, act_dim > 16): the caller keeps the launch-per-step path. */
int lhw_rnn_rollout_policy(LhwRnn* rnn, const float* theta, const float* obs_mean, const float* obs_std, uint64_t seed, uint32_t counter,
                           int deterministic, LhwRolloutLstmPolicy* out, void* stream);
/* BPTT of one minibatch = columns cols[0..B) of the time-major [T][N] rollout (xn / xm [T*N][pad4(obs)] normalised /
 * mirrored observations from lhw_ppo_normalize-compatible layout, done = LHW_DONE_* flags); accumulates grad, stats_dev[0..5] */
int lhw_rnn_grad(LhwRnn* rnn, const float* theta, float* grad, int32_t T, int32_t N, const float* xn, const float* xm,
                 const float* act, const float* old_logp, const float* adv, const float* ret, const uint8_t* done,
                 const int32_t* cols, int32_t B, float* stats_dev, void* stream);
int lhw_rnn_apply(LhwRnn* rnn, float* theta, float* grad, float* adam_m, float* adam_v, int64_t step, float grad_scale,
                  void* stream);
/* Shapes the whole-sequence strip kernels cover (a workgroup of hidden / 32 waves per 32 minibatch rows; the slabs [pad4(obs) + 3 hidden][32]
 * forward and [4 hidden][32] backward must fit the 160 KB of LDS): hidden a multiple of 32 in [MIN_HIDDEN, MAX_HIDDEN], pad4(obs) <= MAX_OBS_PAD.
 * Other shapes keep lhw_rnn_grad's launch-per-step loops. */
#define LHW_LSTM_SEQ_MIN_HIDDEN 32
#define LHW_LSTM_SEQ_MAX_HIDDEN 256
#define LHW_LSTM_SEQ_MAX_OBS_PAD 128
/* Padded observation width up to which lhw_env_rollout_history evaluates the feed-forward actor inside the stepper's wavefronts.  A validated
 * limit, not an LDS size: the rows pass through the stepper's LDS stage region 256 columns at a time (two such pieces still fit the smallest
 * layout beside the two hidden layers, H1's two envs per wave) and the first layer's chains run on from piece to piece, so this is four pieces:
 * history_len <= 27 on jvrc_walk, 26 on jvrc_step, 29 on h1, 23 on h1_walk.  The rollout buffers grow with the row: obs_dev is
 * (T + 1) * N * history_len * base floats and term_obs_dev T * N * history_len * base. */
#define LHW_ROLLOUT_HISTORY_MAX_OBS_PAD 1024
/* Padded input width up to which the LDS-resident strip kernels of the feed-forward MLPs run (csrc/lhw_mlp_strip.hip; hidden width 256): up to 64
 * columns the input slab shares the activation slab with the partial read-out sums (the narrow instantiations); from 68 to this width -- the rows
 * of an observation history -- the input fills the activation slab [256][rows] by itself and the read-out is one chain over k, the order of the
 * per-layer GEMMs and of lhw_env_rollout_history's in-wave step (the wide instantiations; lhw_ppo_debug_set_strip_wide).  A capacity of
 * its own, below LHW_ROLLOUT_HISTORY_MAX_OBS_PAD: wider rows have the resident history rollout, and per-layer GEMMs in the update, in rollout
 * inference and in the critic's values, whatever the switch says. */
#define LHW_MLP_STRIP_MAX_IN_PAD 256
/* debug / A-B: on != 0: lhw_rnn_grad runs each network's forward time loop and its BPTT time loop (rl/algos/ppo.py:512-533) as ONE launch each
 * (the whole-sequence strip kernels, the critic's on a side stream) where the shape is covered; 0: four launches per time step and network.
 * Same bits either way.  A new handle takes the environment's LHW_RNN_SEQ_FUSED (default 1: the A/B of DESIGN.md 4.2c). */
int lhw_rnn_debug_set_seq_fused(LhwRnn* rnn, int32_t on);
/* test hook: 1 if the last lhw_rnn_grad of this handle ran the whole-sequence strip kernels, 0 if the launch-per-step loops */
int lhw_rnn_debug_last_grad_fused(const LhwRnn* rnn);
/* lhw_ppo_debug_grad_sqnorms for the recurrent handle (the norms of the last lhw_rnn_apply) */
int lhw_rnn_debug_grad_sqnorms(LhwRnn* rnn, float* out2_host);
/* xn (and xm) for the recurrent path: same as lhw_ppo_normalize but on an LhwRnn handle */
int lhw_rnn_normalize(LhwRnn* rnn, const float* obs, int64_t R, const float* obs_mean, const float* obs_std, float* xn,
                      float* xm, void* stream);

/* Headless eval frames: the rendering half of the reference's eval (rl/utils/eval.py:38-67: a 640 x 480 tracking camera on the robot,
 * mujoco.Renderer.update_scene / render once per control step, the frames written as a video) as a ray caster for the analytic
 * primitives the model loader accepts (mjtGeom values of lhw_model_fields.h's geom_type: plane 0, sphere 2, capsule 3, ellipsoid 4,
 * cylinder 5, box 6; geom_size as MuJoCo's: sphere r; capsule / cylinder r, half length along local z; ellipsoid semi-axes; box half
 * extents; a plane is infinite).  No GL, no CPU MuJoCo, no pixel parity with MuJoCo's renderer: the camera model and the shading are
 * the ones stated here.  Pixel (x, y) of a W x H image, y growing downwards, looks along
 *   d = normalize(forward + tan(fovy / 2) * ((2 (x + 0.5) / W - 1) * W / H * right - (2 (y + 0.5) / H - 1) * up)). */
typedef struct {
  int32_t width, height;        /* pixels, any value >= 1 (edge tiles are clipped) */
  float   fovy_deg;             /* vertical field of view; default 45 */
  float   light_dir[3];         /* unit vector towards the light, world frame */
  float   ambient, diffuse;     /* colour = rgb * (ambient + diffuse * max(0, n.l) * lit) */
  float   background[3];
  float   checker_size;         /* > 0: planes get a checkerboard of this cell size (second colour = 0.8 * rgb); 0: none */
  int32_t shadows;              /* != 0: one shadow ray towards light_dir, origin = hit + 1e-3 m * n */
  int32_t cull;                 /* != 0 (default): per-tile geom culling; 0: every tile tests every geom (test hook, same bits) */
} LhwRenderSettings;
#define LHW_RENDER_MAX_GEOMS 64
/* F frames of G geoms in one launch, one wavefront per 8 x 8 pixel tile of one frame.  All pointers are device buffers; the call keeps
 * no state and works on any stream.  geom_pos is RELATIVE TO THE FRAME'S CAMERA POSITION (the host subtracts in float64 before it casts:
 * a robot 50 m from the origin renders like one at the origin); geom_mat is the geom's world rotation, row-major (columns = local axes).
 * cam[f] = the rows right, up, forward of the camera frame (9), the camera's world x, y reduced modulo 2 * checker_size in float64 (2:
 * the checkerboard is anchored to the world), one pad.  A geom with rgba alpha 0 is not drawn and casts no shadow.  Outputs: rgb 8-bit
 * (channel = floor(255 * min(1, c) + 0.5)); hit = geom_id * 8 + surface part (box face 0..5 = -x +x -y +y -z +z; capsule 0 body, 1 the
 * cap at -z, 2 at +z; cylinder 0 body, 1 the disc at -z, 2 at +z; 0 otherwise), -1 for background; depth = the ray parameter t of the
 * unit direction d, +inf for background.  Planes are two-sided (the normal is flipped towards the viewer); only hits with t > 0 count.
 * G > LHW_RENDER_MAX_GEOMS: LHW_ERR_UNSUPPORTED; a non-positive image size, field of view or drawn geom size, an unknown geom type:
 * LHW_ERR_ARG -- with nothing written (the type and size tables are read back once: the call synchronises `stream` before it launches). */
int lhw_render_frames(const LhwRenderSettings* s, int32_t G, const int32_t* geom_type_dev /*[G]*/, const float* geom_size_dev /*[G][3]*/,
                      const float* geom_rgba_dev /*[G][4], alpha 0 = not drawn*/, int32_t F, const float* geom_pos_dev /*[F][G][3]*/,
                      const float* geom_mat_dev /*[F][G][9]*/, const float* cam_dev /*[F][12]*/, uint8_t* rgb_dev /*[F][H][W][3]*/,
                      int32_t* hit_dev /*[F][H][W], nullable*/, float* depth_dev /*[F][H][W], nullable*/, void* stream);

/* lhw_render_frames with per-frame geoms, more of them, translucency and a cone: the task markers and the stepping terrain of the
 * reference's eval (envs/jvrc/jvrc_step.py:78-198 draw_markers, tasks/stepping_task.py:320-334).  Camera model, ray, shading formula, the
 * 8 x 8 tile per wavefront, camera-relative float32 positions, cam[f], hit parts and byte rounding are those stated above; what is added:
 *
 * Static and dynamic geoms.  A frame draws the G static geoms -- type / size / rgba shared by all F frames, poses per frame, as above --
 * and M dynamic geoms whose type [F][M], size [F][M][3], rgba [F][M][4], pos [F][M][3] (relative to the frame's camera) and mat [F][M][9]
 * are all per frame.  Alpha 0 = absent in this frame.  Geom ids in the outputs: static g -> g, dynamic m -> G + m.  G or M may be 0 and
 * their pointers then NULL.  G + M <= LHW_RENDER_SCENE_MAX_GEOMS, else LHW_ERR_UNSUPPORTED (nothing written); the wave walks them in
 * passes of 64 in id order.  cull = 0 gives the same bits as cull = 1.
 *
 * Alpha.  alpha == 0: not drawn.  0 < alpha < 1: translucent.  Any other value (1 in particular): opaque.  Along a pixel's ray let t_o be
 * the nearest opaque surface (+inf: none); hit / depth / the shadow ray are those of that surface, as above.  Every translucent geom
 * contributes at most ONE layer: its nearest surface point with t > 0, if t < t_o (strictly).  Layer colour = rgb * (ambient + diffuse *
 * max(0, n.l)), planes with the checker rule, n the outward normal of that point (planes: towards the viewer); a layer takes no shadow
 * test, and translucent geoms cast no shadow (shadow rays see every OPAQUE drawn geom, of every pass).  The nearest LHW_RENDER_MAX_LAYERS
 * layers, ordered by t (equal t: the lower geom id in front), are composited front to back over the opaque colour or the background C_o
 * in float32:  C = sum_k a_k c_k prod_{j<k} (1 - a_j) + prod_k (1 - a_k) * C_o;  farther layers are dropped.  Outputs, both nullable:
 * layers = the number of composited layers (0..8), layer_hit = id * 8 + part of the front-most layer, -1 where there is none.
 *
 * Cone, type LHW_RENDER_CONE (render-only, not an mjtGeom value): size (r, hl); axis = local z, the base disc of radius r at z = -hl, the
 * apex at z = +hl.  Part 0 = the lateral surface, part 1 = the base (normal -z).  Lateral normal proportional to (x, y, rho * r / (2 hl)),
 * rho = sqrt(x^2 + y^2); at the apex (0, 0, 1).  Bounding radius for the culling sqrt(r^2 + hl^2).
 *
 * Errors as above, with nothing written: an unknown type or a non-positive needed size (cone: r and hl) of a geom with alpha != 0 -- static,
 * or dynamic in any frame -- is LHW_ERR_ARG.  The static and the dynamic type / size / rgba tables are read back once before the launch. */
#define LHW_RENDER_SCENE_MAX_GEOMS 256
#define LHW_RENDER_MAX_LAYERS 8
#define LHW_RENDER_CONE 32
int lhw_render_scene(const LhwRenderSettings* s, int32_t G, const int32_t* geom_type_dev /*[G]*/, const float* geom_size_dev /*[G][3]*/,
                     const float* geom_rgba_dev /*[G][4]*/, int32_t M, const int32_t* dyn_type_dev /*[F][M]*/, const float* dyn_size_dev /*[F][M][3]*/,
                     const float* dyn_rgba_dev /*[F][M][4]*/, int32_t F, const float* geom_pos_dev /*[F][G][3]*/, const float* geom_mat_dev /*[F][G][9]*/,
                     const float* dyn_pos_dev /*[F][M][3]*/, const float* dyn_mat_dev /*[F][M][9]*/, const float* cam_dev /*[F][12]*/,
                     uint8_t* rgb_dev /*[F][H][W][3]*/, int32_t* hit_dev /*[F][H][W], nullable*/, float* depth_dev /*[F][H][W], nullable*/,
                     int32_t* layers_dev /*[F][H][W], nullable*/, int32_t* layer_hit_dev /*[F][H][W], nullable*/, void* stream);

/* Eval video: a baseline sequential JPEG encoder for the frames above (the reference's eval appends every frame to a video writer,
 * rl/utils/eval.py:25-34, 63).  lhw_jpeg_encode produces, for each of F frames, the ENTROPY-CODED SEGMENT of a baseline JPEG -- every
 * byte between the SOS header and EOI, restart markers included; the host writes the headers (learninghumanoidwalking_amd/video.py).
 * All arithmetic is integer, and this comment is the specification: an independent program that follows it reproduces every byte.
 * Integers are two's complement, >> is the arithmetic shift, / truncates.
 *
 * Settings.  width, height: 1..65535 (the range of a JPEG frame header).  qtable[0] (luminance) and qtable[1] (chrominance): 64 entries
 * each, values 1..255, in NATURAL order (index 8 v + u for vertical frequency v, horizontal frequency u).
 *
 * Colour and sampling.  Three components Y, Cb, Cr, sampled 4:2:0: the MCU covers 16 x 16 pixels and holds six 8 x 8 blocks in the order
 * Y(0,0) Y(8,0) Y(0,8) Y(8,8) Cb Cr (x, y offsets of the block in the MCU).  M = ceil(W / 16) MCUs per MCU row, R = ceil(H / 16) MCU rows.
 * A sample at (x, y) outside the image is the pixel (min(x, W - 1), min(y, H - 1)): the last column and row are replicated.  Per pixel,
 * from its bytes R, G, B (16-bit fixed point, the JFIF matrix):
 *   Y  = ( 19595 R + 38470 G +  7471 B +   32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16          (8421375 = 128 * 65536 + 32767)
 *   Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16
 * all in 0..255.  A chroma sample (i, j) of an MCU is the mean of the Cb (Cr) of the four pixels (2 i + {0, 1}, 2 j + {0, 1}) of the MCU,
 * rounded as (a + b + c + d + 2) >> 2.  Every sample is then level-shifted: s - 128.
 *
 * DCT.  The 8 x 8 forward DCT in the Loeffler-Ligtenberg-Moschytz factorisation with 13-bit constants, rows first, then columns; its
 * output is 8 times the orthonormal 2-D DCT-II.  With D(x, n) = (x + (1 << (n - 1))) >> n, the constants
 *   c1 = 2446 (0.298631336)  c2 = 3196 (0.390180644)  c3 = 4433 (0.541196100)  c4 = 6270 (0.765366865)  c5 = 7373 (0.899976223)
 *   c6 = 9633 (1.175875602)  c7 = 12299 (1.501321110) c8 = 15137 (1.847759065) c9 = 16069 (1.961570560) c10 = 16819 (2.053119869)
 *   c11 = 20995 (2.562915447) c12 = 25172 (3.072711026)                                    (round(8192 x) of the value in brackets)
 * and the eight inputs d0..d7 of one row (pass 1) or column (pass 2), the outputs o0..o7 replace them:
 *   t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4
 *   e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2,  z = (e2 + e3) c3
 *   pass 1: o0 = (e0 + e1) << 2, o4 = (e0 - e1) << 2, o2 = D(z + e3 c4, 11), o6 = D(z - e2 c8, 11)
 *   pass 2: o0 = D(e0 + e1, 2),  o4 = D(e0 - e1, 2),  o2 = D(z + e3 c4, 15), o6 = D(z - e2 c8, 15)
 *   z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) c6,  a3 = z5 - z3 c9, a4 = z5 - z4 c2
 *   o7 = D(t4 c1 - z1 c5 + a3, n), o5 = D(t5 c10 - z2 c11 + a4, n), o3 = D(t6 c12 - z2 c11 + a3, n), o1 = D(t7 c7 - z1 c5 + a4, n)
 *   with n = 11 in pass 1 and 15 in pass 2.
 * Quantisation of the coefficient c at natural index i of a block of component table t, q = qtable[t][i]: sign-symmetric rounding
 * division, k = (|c| + 4 q) / (8 q), the quantised value is k with the sign of c.
 *
 * Entropy coding.  Huffman coding with the four tables of ITU-T T.81 Annex K (K.3 / K.4 DC, K.5 / K.6 AC; luminance tables for Y,
 * chrominance tables for Cb and Cr), coefficients in zig-zag order.  DC: the difference to the previous block OF THE SAME COMPONENT in
 * the restart interval (0 for the first), category s = bit length of |diff|, the code of s, then the s low bits of diff (diff >= 0) or of
 * diff - 1 (diff < 0).  AC: for every non-zero coefficient, ZRL (0xF0) for each full 16 zeros of the run in front of it, then the code of
 * (run << 4) | s and the s bits as for DC; EOB (0x00) closes the block unless coefficient 63 is non-zero.  Bits fill bytes from the most
 * significant bit.  The restart interval is one MCU row (DRI = M).  At the end of every MCU row the last byte is padded with 1-bits; after
 * every MCU row r but the last follow the two bytes FF, D0 + (r mod 8), and the DC predictions restart at 0.  In the coded bytes (the
 * padded ones included, the markers not) every byte FF is followed by a byte 00.
 *
 * Sizes.  A block codes to at most 22 + 63 * 26 = 1660 bits (DC: 11-bit code, 11 bits; each AC: 16-bit code, 10 bits), an MCU row to at
 * most 2 * ceil(6 M * 1660 / 8) stuffed bytes and 2 marker bytes <= LHW_JPEG_MCU_BYTES * M + 4, so
 *   lhw_jpeg_out_bytes     = F * R * (LHW_JPEG_MCU_BYTES * M + 4)          -- the capacity out_dev must have, whatever the content
 *   lhw_jpeg_scratch_bytes = the same + 16 * (F * R + 1)                   -- per MCU row: its staged bytes, its size and its offset
 * (both 0 for F = 0, -1 for bad settings or F < 0).  The call queues three kernels on `stream` -- one wavefront per (frame, MCU row)
 * codes the row into scratch, one scans the row sizes, one packs the rows back to back -- keeps no state and returns without waiting:
 * frame f is out_dev[frame_offset_dev[f] .. frame_offset_dev[f + 1]).  scratch_dev must be 8-byte aligned.
 * Errors, with nothing written: NULL settings or buffers, a size outside 1..65535, F < 0, a table entry outside 1..255, more than
 * 2^31 - 1 MCU rows in all: LHW_ERR_ARG; scratch_bytes or out_capacity below the sizes above: LHW_ERR_ARG, lhw_last_error() names the
 * needed size. */
typedef struct {
  int32_t  width, height;
  uint16_t qtable[2][64];
} LhwJpegSettings;
#define LHW_JPEG_MCU_BYTES 2496      /* 6 blocks * 2 * 208 bytes */
int64_t lhw_jpeg_scratch_bytes(const LhwJpegSettings* s, int32_t F);
int64_t lhw_jpeg_out_bytes(const LhwJpegSettings* s, int32_t F);
int lhw_jpeg_encode(const LhwJpegSettings* s, int32_t F, const uint8_t* rgb_dev /*[F][H][W][3]*/, uint8_t* scratch_dev, int64_t scratch_bytes,
                    uint8_t* out_dev, int64_t out_capacity, int64_t* frame_offset_dev /*[F + 1]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LHW_H */
