// extern "C" entry points of liblhw.so (declared in include/lhw.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lhw.h"
#include "lhw_cartpole.h"
#include "lhw_internal.h"

static thread_local std::string g_err;

int lhw_fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

hipError_t lhw_malloc(void** p, size_t n) {
  static const bool poison = getenv("LHW_POISON") && atoi(getenv("LHW_POISON")) != 0;
  hipError_t e = hipMalloc(p, n);
  if (e == hipSuccess && poison && n) e = hipMemset(*p, 0xFF, n);
  return e;
}

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return lhw_fail(LHW_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_)); \
  } while (0)

struct LhwEnv {
  int task = 0, n_envs = 0, device = 0, nq = 0, nv = 0, nu = 0, obs_dim = 0, act_dim = 0, n_terms = 0;
  std::vector<int32_t> mi;
  std::vector<double> md;
  // cartpole
  CartpoleParams cp{};
  CartpoleState cps{};
  // humanoid
  HumanoidEnv* hum = nullptr;
  double* stage_q = nullptr;  // device staging for get/set state
  double* stage_v = nullptr;
  double* tstat = nullptr;    // the term-statistics block once enabled (kept across a disable; the kernels see it through set_term_stats_block)
  LhwDevMem mem;              // the cartpole state, the staging buffers and the term statistics (the humanoid stepper owns the rest of its own)
};

extern "C" int lhw_version(void) { return 1; }
extern "C" const char* lhw_last_error(void) { return g_err.c_str(); }

static const int32_t* IFLD(const LhwEnv* e, int f) { return e->mi.data() + e->mi[LHW_IH_COUNT + f]; }
static const double* DFLD(const LhwEnv* e, int f) { return e->md.data() + e->mi[LHW_IH_COUNT + LHW_IF_COUNT + f]; }

static int check_model(const int32_t* mi, int64_t ni, const double* md, int64_t nd) {
  if (!mi || !md || ni < LHW_IH_COUNT + LHW_IF_COUNT + LHW_DF_COUNT || nd < LHW_DH_COUNT)
    return lhw_fail(LHW_ERR_MODEL, "model blobs too small");
  if ((uint32_t)mi[LHW_IH_MAGIC] != LHW_MODEL_MAGIC || mi[LHW_IH_VERSION] != LHW_MODEL_VERSION)
    return lhw_fail(LHW_ERR_MODEL, "bad model magic/version");
  if (mi[LHW_IH_N_IFIELDS] != LHW_IF_COUNT || mi[LHW_IH_N_DFIELDS] != LHW_DF_COUNT)
    return lhw_fail(LHW_ERR_MODEL, "model field table does not match this build");
  for (int f = 0; f < LHW_IF_COUNT; f++)
    if (mi[LHW_IH_COUNT + f] < 0 || mi[LHW_IH_COUNT + f] > ni) return lhw_fail(LHW_ERR_MODEL, "int field %d offset out of range", f);
  for (int f = 0; f < LHW_DF_COUNT; f++)
    if (mi[LHW_IH_COUNT + LHW_IF_COUNT + f] < 0 || mi[LHW_IH_COUNT + LHW_IF_COUNT + f] > nd)
      return lhw_fail(LHW_ERR_MODEL, "double field %d offset out of range", f);
  return LHW_OK;
}

// getsolparam (engine_core_constraint.c): refsafe + clamps
static void solparam(const LhwEnv* e, const double* sr, const double* si, double* solref, double* solimp) {
  const double h = e->md[LHW_DH_TIMESTEP];
  solref[0] = sr[0]; solref[1] = sr[1];
  for (int k = 0; k < 5; k++) solimp[k] = si[k];
  if (!(e->mi[LHW_IH_DISABLEFLAGS] & (1 << 11)) && solref[0] > 0 && solref[0] < 2 * h) solref[0] = 2 * h;
  solimp[0] = fmin(0.9999, fmax(0.0001, solimp[0]));
  solimp[1] = fmin(0.9999, fmax(0.0001, solimp[1]));
  solimp[2] = fmax(0.0, solimp[2]);
  solimp[3] = fmin(0.9999, fmax(0.0001, solimp[3]));
  solimp[4] = fmax(1.0, solimp[4]);
}

static int create_cartpole(LhwEnv* e, const LhwEnvConfig* cfg) {
  // the lane-per-env kernel is specialised to the slide-x / hinge-y topology of the reference's cartpole.xml
  const int32_t* jt = IFLD(e, LHW_IF_JNT_TYPE);
  const double* ax = DFLD(e, LHW_DF_JNT_AXIS);
  if (e->nq != 2 || e->nv != 2 || e->nu != 1 || e->mi[LHW_IH_NBODY] != 3 || jt[0] != 2 || jt[1] != 3)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "cartpole task needs a 2-dof slide+hinge model");
  if (fabs(ax[0] - 1) > 1e-12 || fabs(ax[4] - 1) > 1e-12) return lhw_fail(LHW_ERR_UNSUPPORTED, "cartpole axes must be slide x / hinge y");
  const double* ipos = DFLD(e, LHW_DF_BODY_IPOS);
  const double* bpos = DFLD(e, LHW_DF_BODY_POS);
  const double* jpos = DFLD(e, LHW_DF_JNT_POS);
  const double* iq = DFLD(e, LHW_DF_BODY_IQUAT);
  for (int k = 0; k < 6; k++)
    if (fabs(bpos[3 + k]) > 1e-12 || fabs(jpos[k]) > 1e-12) return lhw_fail(LHW_ERR_UNSUPPORTED, "cartpole bodies/joints must sit at the origin");
  if (fabs(ipos[6]) > 1e-12 || fabs(ipos[7]) > 1e-12 || fabs(iq[8] - 1) > 1e-12)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "pole inertial frame must lie on the local z axis, axis-aligned");
  if (e->mi[LHW_IH_NPAIR] != 0) return lhw_fail(LHW_ERR_UNSUPPORTED, "cartpole kernel has no contact support");
  if (cfg->frame_skip <= 0) return lhw_fail(LHW_ERR_ARG, "frame_skip must be positive");
  CartpoleParams& p = e->cp;
  const double* mass = DFLD(e, LHW_DF_BODY_MASS);
  const double* inertia = DFLD(e, LHW_DF_BODY_INERTIA);
  p.n_envs = e->n_envs; p.frame_skip = cfg->frame_skip; p.max_traj_len = cfg->max_traj_len;
  p.iterations = e->mi[LHW_IH_ITERATIONS];
  p.warmstart = !(e->mi[LHW_IH_DISABLEFLAGS] & (1 << 7));
  p.eulerdamp = !(e->mi[LHW_IH_DISABLEFLAGS] & (1 << 14));
  p.env_id_base = (uint32_t)cfg->env_id_base; p.seed = cfg->seed;
  p.mc = mass[1]; p.mp = mass[2]; p.l = ipos[8]; p.Iyy = inertia[7];
  const double *arm = DFLD(e, LHW_DF_DOF_ARMATURE), *damp = DFLD(e, LHW_DF_DOF_DAMPING);
  p.arm[0] = arm[0]; p.arm[1] = arm[1]; p.damp[0] = damp[0]; p.damp[1] = damp[1];
  p.gear = DFLD(e, LHW_DF_ACTUATOR_GEAR)[0];
  if (IFLD(e, LHW_IF_ACTUATOR_CTRLLIMITED)[0] || IFLD(e, LHW_IF_ACTUATOR_FORCELIMITED)[0])
    return lhw_fail(LHW_ERR_UNSUPPORTED, "cartpole kernel assumes an unlimited motor");
  if (IFLD(e, LHW_IF_ACTUATOR_TRNID)[0] != 0) return lhw_fail(LHW_ERR_UNSUPPORTED, "motor must drive the slider");
  if (DFLD(e, LHW_DF_DOF_FRICTIONLOSS)[0] != 0 || DFLD(e, LHW_DF_DOF_FRICTIONLOSS)[1] != 0)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "cartpole kernel has no frictionloss support");
  p.h = e->md[LHW_DH_TIMESTEP];
  if (e->md[LHW_DH_GRAVITY_X] != 0 || e->md[LHW_DH_GRAVITY_Y] != 0) return lhw_fail(LHW_ERR_UNSUPPORTED, "gravity must be along z");
  p.g = -e->md[LHW_DH_GRAVITY_Z];
  const int32_t* lim = IFLD(e, LHW_IF_JNT_LIMITED);
  if (lim[1]) return lhw_fail(LHW_ERR_UNSUPPORTED, "hinge limit not supported by the cartpole kernel");
  const double* rng = DFLD(e, LHW_DF_JNT_RANGE);
  if (lim[0]) { p.range_lo = rng[0]; p.range_hi = rng[1]; } else { p.range_lo = -1e300; p.range_hi = 1e300; }
  p.margin = DFLD(e, LHW_DF_JNT_MARGIN)[0];
  solparam(e, DFLD(e, LHW_DF_JNT_SOLREF), DFLD(e, LHW_DF_JNT_SOLIMP), p.solref, p.solimp);
  p.invweight0 = DFLD(e, LHW_DF_DOF_INVWEIGHT0)[0];
  p.meaninertia = e->md[LHW_DH_MEANINERTIA]; p.tolerance = e->md[LHW_DH_TOLERANCE];
  p.kp = cfg->kp ? cfg->kp[0] : 0; p.kd = cfg->kd ? cfg->kd[0] : 0;
  e->obs_dim = 5; e->act_dim = 1; e->n_terms = 4;
  const size_t N = e->n_envs;
  e->cps.d = e->mem.get<double>(CARTPOLE_NFIELDS * N);
  e->cps.traj_len = e->mem.get<int32_t>(N);
  e->cps.reset_count = e->mem.get<uint32_t>(N);
  e->cps.ep_stats = e->mem.get<double>(3);
  return e->mem.failed() ? lhw_fail(LHW_ERR_HIP, "cartpole state allocation failed (n_envs=%d)", e->n_envs) : LHW_OK;
}

extern "C" int lhw_env_create(const int32_t* model_i, int64_t n_model_i, const double* model_d, int64_t n_model_d,
                              const LhwEnvConfig* cfg, LhwEnv** out) {
  if (!cfg || !out) return lhw_fail(LHW_ERR_ARG, "null argument");
  *out = nullptr;
  int rc = check_model(model_i, n_model_i, model_d, n_model_d);
  if (rc) return rc;
  if (cfg->n_envs <= 0) return lhw_fail(LHW_ERR_ARG, "n_envs must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return lhw_fail(LHW_ERR_NO_DEVICE, "no HIP device visible: liblhw has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return lhw_fail(LHW_ERR_ARG, "device %d out of range (%d visible)", cfg->device, ndev);
  HIPCHK(hipSetDevice(cfg->device));
  LhwEnv* e = new LhwEnv();
  e->mi.assign(model_i, model_i + n_model_i);
  e->md.assign(model_d, model_d + n_model_d);
  e->task = cfg->task; e->n_envs = cfg->n_envs; e->device = e->mem.device = cfg->device;
  e->nq = model_i[LHW_IH_NQ]; e->nv = model_i[LHW_IH_NV]; e->nu = model_i[LHW_IH_NU];
  if (cfg->task == LHW_TASK_CARTPOLE) rc = create_cartpole(e, cfg);
  else if (cfg->task == LHW_TASK_JVRC_WALK || cfg->task == LHW_TASK_H1_STAND || cfg->task == LHW_TASK_JVRC_STEP || cfg->task == LHW_TASK_H1_WALK) rc = humanoid_create(&e->hum, e->mi, e->md, cfg, &e->obs_dim, &e->act_dim, &e->n_terms);
  else rc = lhw_fail(LHW_ERR_ARG, "unknown task %d", cfg->task);
  if (rc == LHW_OK) {
    e->stage_q = e->mem.get<double>((size_t)e->n_envs * e->nq, LhwDevMem::RAW);
    e->stage_v = e->mem.get<double>((size_t)e->n_envs * e->nv, LhwDevMem::RAW);
    if (e->mem.failed()) rc = lhw_fail(LHW_ERR_HIP, "lhw_malloc(staging) failed");
  }
  if (rc != LHW_OK) { lhw_env_destroy(e); return rc; }
  *out = e;
  return LHW_OK;
}

extern "C" int lhw_env_destroy(LhwEnv* e) {
  if (!e) return LHW_OK;
  humanoid_destroy(e->hum);
  delete e;
  return LHW_OK;
}

extern "C" int lhw_env_obs_dim(const LhwEnv* e) { return e ? e->obs_dim : LHW_ERR_ARG; }
extern "C" int lhw_env_act_dim(const LhwEnv* e) { return e ? e->act_dim : LHW_ERR_ARG; }
extern "C" int lhw_env_num_reward_terms(const LhwEnv* e) { return e ? e->n_terms : LHW_ERR_ARG; }
extern "C" int lhw_env_nq(const LhwEnv* e) { return e ? e->nq : LHW_ERR_ARG; }
extern "C" int lhw_env_nv(const LhwEnv* e) { return e ? e->nv : LHW_ERR_ARG; }

extern "C" int lhw_env_reset(LhwEnv* e, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  HIPCHK(hipSetDevice(e->device));
  if (e->task == LHW_TASK_CARTPOLE) cartpole_launch_reset(e->cp, e->cps, mask_dev, obs_dev, (hipStream_t)stream);
  else humanoid_reset(e->hum, mask_dev, obs_dev, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

extern "C" int lhw_env_step(LhwEnv* e, const float* act_dev, float* obs_dev, float* term_obs_dev, float* rew_dev,
                            uint8_t* done_dev, float* rew_terms_dev, void* stream) {
  if (!e || !act_dev || !obs_dev || !rew_dev || !done_dev) return lhw_fail(LHW_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(e->device));
  if (e->task == LHW_TASK_CARTPOLE)
    cartpole_launch_step(e->cp, e->cps, act_dev, obs_dev, term_obs_dev, rew_dev, done_dev, rew_terms_dev, (hipStream_t)stream);
  else humanoid_step(e->hum, act_dev, obs_dev, term_obs_dev, rew_dev, done_dev, rew_terms_dev, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

extern "C" int lhw_env_step_range(LhwEnv* e, int32_t first, int32_t count, const float* act_dev, float* obs_dev, float* term_obs_dev,
                                  float* rew_dev, uint8_t* done_dev, float* rew_terms_dev, void* stream) {
  if (!e || !act_dev || !obs_dev || !rew_dev || !done_dev) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (e->task == LHW_TASK_CARTPOLE) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_step_range: the lane-per-env cartpole stepper advances whole batches");
  HIPCHK(hipSetDevice(e->device));
  if (humanoid_step_range(e->hum, first, count, act_dev, obs_dev, term_obs_dev, rew_dev, done_dev, rew_terms_dev, (hipStream_t)stream))
    return lhw_fail(LHW_ERR_ARG, "env range [%d, %d) outside the batch", first, first + count);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

// What the five resident-rollout entry points share, once: the argument checks, the launch (humanoid_rollout) and its codes.  `name`: the entry
// point that was called.
static int env_rollout(const char* name, LhwEnv* e, const HumanoidRollout& rq, void* stream) {
  if (!e || (!rq.mlp && !rq.lstm) || !rq.obs || !rq.act || !rq.logp || !rq.term_obs || !rq.rew || !rq.done ||
      (rq.kind == POLICY_LSTM && !rq.reset0))
    return lhw_fail(LHW_ERR_ARG, "null argument");
  if (e->task == LHW_TASK_CARTPOLE) return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: wave-per-env (humanoid) steppers only", name);
  if (rq.stin_all && e->task != LHW_TASK_JVRC_STEP) return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: the stepping record needs a stepping-task env", name);
  if (rq.stin_all && !rq.tin_all) return lhw_fail(LHW_ERR_ARG, "%s: the stepping record is exported together with the task-input record", name);
  HIPCHK(hipSetDevice(e->device));
  const int rc = humanoid_rollout(e->hum, rq, (hipStream_t)stream);
  if (rc == -1) return lhw_fail(LHW_ERR_ARG, "env range [%d, %d) outside the batch, or T = %d", rq.first, rq.first + rq.count, rq.T);
  if (rc == -4) return lhw_fail(LHW_ERR_HIP, "%s: a HIP call failed while preparing the launch (%s)", name, hipGetErrorString(hipGetLastError()));
  if (rc == -5)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: a diagnostic clock of this env is armed (lhw_env_phase_cycles / lhw_env_debug_wave_cycles) and only the plain feed-forward "
                                         "rollout kernels carry the clocks: step this env launch by launch (lhw_env_step)", name);
  if (rc == -6)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: the actuator randomisation of this env is armed (lhw_env_set_actuator_randomization) and only the feed-forward "
                                         "rollout kernels without a history carry it: step this env launch by launch (lhw_env_step)", name);
  if (rc && rq.kind == POLICY_MLP)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: needs a float32 actor obs %d -> 256 -> 256 -> act %d (<= 12) and a model that fits the task's resident kernel", name,
                    e->obs_dim, e->act_dim);
  if (rc && rq.kind == POLICY_HIST)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: needs a float32 actor obs %d x %d (padded <= %d) -> 256 -> 256 -> act %d (<= 12) and a model that fits the task's "
                    "resident kernel", name, rq.history_len, e->obs_dim, LHW_ROLLOUT_HISTORY_MAX_OBS_PAD, e->act_dim);
  if (rc) return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: needs a float32 LSTM actor obs %d -> 256 -> 256 -> act %d (<= 12) with a state row per env and a model that fits "
                          "the task's resident kernel", name, e->obs_dim, e->act_dim);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
// the arguments the five entry points share, in the ABI's order, as a request of a feed-forward policy without a history; the entry point names the rest
static HumanoidRollout rollout_request(int32_t first, int32_t count, int32_t T, float* obs_dev, float* act_dev, float* logp_dev, float* term_obs_dev, float* rew_dev,
                                       uint8_t* done_dev, float* rew_terms_dev, double* tin_dev, double* stin_dev) {
  HumanoidRollout rq;
  rq.first = first; rq.count = count; rq.T = T;
  rq.obs = obs_dev; rq.act = act_dev; rq.logp = logp_dev; rq.term_obs = term_obs_dev; rq.rew = rew_dev; rq.done = done_dev; rq.rew_terms = rew_terms_dev;
  rq.tin_all = tin_dev; rq.stin_all = stin_dev;
  return rq;
}
extern "C" int lhw_env_rollout(LhwEnv* e, const LhwRolloutPolicy* policy, int32_t first, int32_t count, int32_t T, float* obs_dev, float* act_dev,
                               float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev, float* rew_terms_dev, void* stream) {
  HumanoidRollout rq = rollout_request(first, count, T, obs_dev, act_dev, logp_dev, term_obs_dev, rew_dev, done_dev, rew_terms_dev, nullptr, nullptr);
  rq.mlp = policy;
  return env_rollout("lhw_env_rollout", e, rq, stream);
}
extern "C" int lhw_env_rollout_task_inputs(LhwEnv* e, const LhwRolloutPolicy* policy, int32_t first, int32_t count, int32_t T, float* obs_dev, float* act_dev,
                                           float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev, float* rew_terms_dev, double* tin_dev,
                                           void* stream) {
  if (!tin_dev) return lhw_fail(LHW_ERR_ARG, "lhw_env_rollout_task_inputs: null task-input buffer");
  HumanoidRollout rq = rollout_request(first, count, T, obs_dev, act_dev, logp_dev, term_obs_dev, rew_dev, done_dev, rew_terms_dev, tin_dev, nullptr);
  rq.mlp = policy;
  return env_rollout("lhw_env_rollout_task_inputs", e, rq, stream);
}
extern "C" int lhw_env_rollout_step_task_inputs(LhwEnv* e, const LhwRolloutPolicy* policy, int32_t first, int32_t count, int32_t T, float* obs_dev,
                                                float* act_dev, float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev,
                                                float* rew_terms_dev, double* tin_dev, double* stin_dev, void* stream) {
  if (!tin_dev || !stin_dev) return lhw_fail(LHW_ERR_ARG, "lhw_env_rollout_step_task_inputs: null task-input buffer");
  HumanoidRollout rq = rollout_request(first, count, T, obs_dev, act_dev, logp_dev, term_obs_dev, rew_dev, done_dev, rew_terms_dev, tin_dev, stin_dev);
  rq.mlp = policy;
  return env_rollout("lhw_env_rollout_step_task_inputs", e, rq, stream);
}

extern "C" int lhw_env_rollout_history(LhwEnv* e, const LhwRolloutPolicy* policy, int32_t first, int32_t count, int32_t T, int32_t history_len, float* obs_dev,
                                       float* act_dev, float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev, float* rew_terms_dev,
                                       double* tin_dev, double* stin_dev, void* stream) {
  if (history_len < 1) return lhw_fail(LHW_ERR_ARG, "lhw_env_rollout_history: history_len = %d", history_len);
  HumanoidRollout rq = rollout_request(first, count, T, obs_dev, act_dev, logp_dev, term_obs_dev, rew_dev, done_dev, rew_terms_dev, tin_dev, stin_dev);
  rq.mlp = policy;
  rq.history_len = history_len;
  if (history_len > 1) rq.kind = POLICY_HIST;   // (history_len = 1, no history: the kernels of lhw_env_rollout)
  return env_rollout("lhw_env_rollout_history", e, rq, stream);
}

extern "C" int lhw_env_rollout_lstm(LhwEnv* e, const LhwRolloutLstmPolicy* policy, int32_t first, int32_t count, int32_t T, float* obs_dev, float* act_dev,
                                    float* logp_dev, float* term_obs_dev, float* rew_dev, uint8_t* done_dev, float* rew_terms_dev, const uint8_t* reset0_dev,
                                    double* tin_dev, double* stin_dev, void* stream) {
  HumanoidRollout rq = rollout_request(first, count, T, obs_dev, act_dev, logp_dev, term_obs_dev, rew_dev, done_dev, rew_terms_dev, tin_dev, stin_dev);
  rq.kind = POLICY_LSTM;
  rq.lstm = policy;
  rq.reset0 = reset0_dev;
  return env_rollout("lhw_env_rollout_lstm", e, rq, stream);
}

extern "C" int lhw_env_last_rollout_queued(LhwEnv* e) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  return e->task == LHW_TASK_CARTPOLE ? 0 : humanoid_last_rollout_queued(e->hum);
}

extern "C" int lhw_env_get_state(LhwEnv* e, double* qpos_host, double* qvel_host) {
  if (!e || !qpos_host || !qvel_host) return lhw_fail(LHW_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  if (e->task == LHW_TASK_CARTPOLE) cartpole_launch_get_state(e->cp, e->cps, e->stage_q, e->stage_v, 0);
  else humanoid_get_state(e->hum, e->stage_q, e->stage_v, 0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(qpos_host, e->stage_q, sizeof(double) * (size_t)e->n_envs * e->nq, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(qvel_host, e->stage_v, sizeof(double) * (size_t)e->n_envs * e->nv, hipMemcpyDeviceToHost));
  return LHW_OK;
}

extern "C" int lhw_env_set_state(LhwEnv* e, const double* qpos_host, const double* qvel_host) {
  if (!e || !qpos_host || !qvel_host) return lhw_fail(LHW_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(e->stage_q, qpos_host, sizeof(double) * (size_t)e->n_envs * e->nq, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->stage_v, qvel_host, sizeof(double) * (size_t)e->n_envs * e->nv, hipMemcpyHostToDevice));
  if (e->task == LHW_TASK_CARTPOLE) cartpole_launch_set_state(e->cp, e->cps, e->stage_q, e->stage_v, 0);
  else humanoid_set_state(e->hum, e->stage_q, e->stage_v, 0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return LHW_OK;
}

extern "C" int lhw_env_get_task_shaping(const LhwEnv* e, double* term_weights, double* term_limits) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  if (!e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "task shaping exists for the humanoid tasks only");
  double w[LHW_MAX_REWARD_TERMS];
  humanoid_get_task_shaping(e->hum, w, term_limits);
  for (int k = 0; term_weights && k < e->n_terms; k++) term_weights[k] = w[k];
  return LHW_OK;
}

extern "C" int lhw_env_set_task_shaping(LhwEnv* e, const double* term_weights, int32_t n_weights, const double* term_limits, int32_t n_limits) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  if (!e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "task shaping exists for the humanoid tasks only");
  if (term_weights) {
    if (n_weights != e->n_terms) return lhw_fail(LHW_ERR_ARG, "lhw_env_set_task_shaping: n_weights = %d, this task has %d reward terms", (int)n_weights, e->n_terms);
    for (int k = 0; k < n_weights; k++)
      if (!std::isfinite(term_weights[k])) return lhw_fail(LHW_ERR_ARG, "lhw_env_set_task_shaping: weight %d is not finite", k);
  }
  if (term_limits) {
    if (n_limits != LHW_TERM_LIMIT_COUNT) return lhw_fail(LHW_ERR_ARG, "lhw_env_set_task_shaping: n_limits = %d, must be %d (lower, upper)", (int)n_limits, LHW_TERM_LIMIT_COUNT);
    if (std::isnan(term_limits[0]) || std::isnan(term_limits[1])) return lhw_fail(LHW_ERR_ARG, "lhw_env_set_task_shaping: a termination limit is NaN");
    if (!(term_limits[0] < term_limits[1]))
      return lhw_fail(LHW_ERR_ARG, "lhw_env_set_task_shaping: lower limit %g is not below upper limit %g", term_limits[0], term_limits[1]);
    if (e->task == LHW_TASK_JVRC_STEP && term_limits[1] != (double)INFINITY)
      return lhw_fail(LHW_ERR_ARG, "lhw_env_set_task_shaping: the stepping task has no upper limit (pass +inf, got %g)", term_limits[1]);
  }
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  if (humanoid_set_task_shaping(e->hum, term_weights, n_weights, term_limits)) return lhw_fail(LHW_ERR_HIP, "task shaping: parameter upload failed");
  return LHW_OK;
}

// ep_stats[first .. first + count) -> host after a device synchronise, then cleared on the device
static int pop_stats(LhwEnv* e, int first, int count, double* out) {
  HIPCHK(hipSetDevice(e->device));
  double* dev = (e->task == LHW_TASK_CARTPOLE ? e->cps.ep_stats : humanoid_ep_stats(e->hum)) + first;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, dev, sizeof(double) * count, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(dev, 0, sizeof(double) * count));
  return LHW_OK;
}

extern "C" int lhw_env_get_actuator_randomization(LhwEnv* e, LhwActuatorRand* out) {
  if (!e || !out) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (!e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_get_actuator_randomization: the actuator randomisation exists for the humanoid tasks only");
  humanoid_get_actuator_rand(e->hum, out);
  return LHW_OK;
}

extern "C" int lhw_env_set_actuator_randomization(LhwEnv* e, const LhwActuatorRand* a) {
  if (!e || !a) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (!e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_set_actuator_randomization: the actuator randomisation exists for the humanoid tasks only");
  const char* fn = "lhw_env_set_actuator_randomization";
  if (!std::isfinite(a->pdrand_k) || a->pdrand_k < 0 || a->pdrand_k >= 1) return lhw_fail(LHW_ERR_ARG, "%s: pdrand_k = %g, must lie in [0, 1)", fn, a->pdrand_k);
  if (a->bemf_interval < 1) return lhw_fail(LHW_ERR_ARG, "%s: bemf_interval = %d, must be >= 1", fn, (int)a->bemf_interval);
  if (!std::isfinite(a->bemf_lo) || a->bemf_lo < 0) return lhw_fail(LHW_ERR_ARG, "%s: bemf_lo = %g, must be finite and >= 0", fn, a->bemf_lo);
  if (!std::isfinite(a->bemf_hi) || a->bemf_lo > a->bemf_hi) return lhw_fail(LHW_ERR_ARG, "%s: bemf_hi = %g, must be finite and >= bemf_lo = %g", fn, a->bemf_hi, a->bemf_lo);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  const int rc = humanoid_set_actuator_rand(e->hum, a);
  if (rc == -2)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: a diagnostic clock of this env is armed (lhw_env_phase_cycles / lhw_env_debug_wave_cycles) and the kernels that "
                                         "carry the actuator randomisation carry no clocks", fn);
  return rc ? lhw_fail(LHW_ERR_HIP, "%s: parameter upload failed", fn) : LHW_OK;
}

extern "C" int lhw_env_get_bemf_damping(LhwEnv* e, double* tau_d_host) {
  if (!e || !tau_d_host) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (!e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_get_bemf_damping: the actuator randomisation exists for the humanoid tasks only");
  HIPCHK(hipSetDevice(e->device));
  if (humanoid_bemf_damping(e->hum, tau_d_host)) return lhw_fail(LHW_ERR_HIP, "lhw_env_get_bemf_damping: copy failed");
  return LHW_OK;
}

// which tasks have a command: the walking tasks and the stepping task (the latter no pin)
static int commands_supported(const LhwEnv* e, const char* fn, bool pin) {
  if (!e->hum || e->task == LHW_TASK_H1_STAND)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: this task has no command (task commands exist for jvrc_walk, h1_walk and jvrc_step)", fn);
  if (pin && e->task == LHW_TASK_JVRC_STEP)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: the stepping task's command is a footstep plan; only the walking tasks' commands can be pinned", fn);
  return LHW_OK;
}

extern "C" int lhw_env_get_task_commands(const LhwEnv* e, LhwTaskCommands* out) {
  if (!e || !out) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (const int rc = commands_supported(e, "lhw_env_get_task_commands", false)) return rc;
  humanoid_get_task_commands(e->hum, out);
  return LHW_OK;
}

extern "C" int lhw_env_set_task_commands(LhwEnv* e, const LhwTaskCommands* c) {
  if (!e || !c) return lhw_fail(LHW_ERR_ARG, "null argument");
  const char* fn = "lhw_env_set_task_commands";
  if (const int rc = commands_supported(e, fn, false)) return rc;
  const struct { const char* name; const double* v; } ranges[3] = {{"inplace_yaw", c->inplace_yaw}, {"forward_vx", c->forward_vx}, {"forward_vy", c->forward_vy}};
  for (const auto& r : ranges) {
    if (!std::isfinite(r.v[0]) || !std::isfinite(r.v[1])) return lhw_fail(LHW_ERR_ARG, "%s: %s = (%g, %g) is not finite", fn, r.name, r.v[0], r.v[1]);
    if (r.v[0] > r.v[1]) return lhw_fail(LHW_ERR_ARG, "%s: %s = (%g, %g), lo must not exceed hi", fn, r.name, r.v[0], r.v[1]);
  }
  const struct { const char* name; const double* v; int n; } cdfs[2] = {{"mode_cdf", c->mode_cdf, 2}, {"step_mode_cdf", c->step_mode_cdf, 4}};
  for (const auto& d : cdfs)
    for (int k = 0; k < d.n; k++) {
      const double lo = k ? d.v[k - 1] : 0.0;
      if (!(d.v[k] >= lo && d.v[k] <= 1.0))   // (NaN fails it too)
        return lhw_fail(LHW_ERR_ARG, "%s: %s[%d] = %g, the cumulative thresholds must ascend within [0, 1]", fn, d.name, k, d.v[k]);
    }
  if (c->switch_stand_every < 0) return lhw_fail(LHW_ERR_ARG, "%s: switch_stand_every = %d, must be >= 0 (0: never)", fn, (int)c->switch_stand_every);
  if (c->switch_walk_every < 0) return lhw_fail(LHW_ERR_ARG, "%s: switch_walk_every = %d, must be >= 0 (0: never)", fn, (int)c->switch_walk_every);
  if (!std::isfinite(c->step_height_start)) return lhw_fail(LHW_ERR_ARG, "%s: step_height_start = %g is not finite", fn, c->step_height_start);
  if (!std::isfinite(c->step_height_span) || c->step_height_span <= 0) return lhw_fail(LHW_ERR_ARG, "%s: step_height_span = %g, must be finite and > 0", fn, c->step_height_span);
  if (!std::isfinite(c->step_height_max)) return lhw_fail(LHW_ERR_ARG, "%s: step_height_max = %g is not finite", fn, c->step_height_max);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  if (humanoid_set_task_commands(e->hum, c)) return lhw_fail(LHW_ERR_HIP, "%s: parameter upload failed", fn);
  return LHW_OK;
}

extern "C" int lhw_env_pin_commands(LhwEnv* e, int32_t first, int32_t count, const int32_t* mode_host, const double* ref_host) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  const char* fn = "lhw_env_pin_commands";
  if (const int rc = commands_supported(e, fn, true)) return rc;
  if (first < 0 || count < 0 || (int64_t)first + count > e->n_envs)
    return lhw_fail(LHW_ERR_ARG, "%s: envs [first = %d, first + count = %lld) lie outside the batch of %d", fn, (int)first, (long long)first + count, e->n_envs);
  if (count > 0 && (!mode_host || !ref_host)) return lhw_fail(LHW_ERR_ARG, "%s: null mode / ref array", fn);
  for (int i = 0; i < count; i++) {
    if (mode_host[i] < -1 || mode_host[i] > 2) return lhw_fail(LHW_ERR_ARG, "%s: mode[%d] = %d, must be -1 (free), 0 STANDING, 1 INPLACE or 2 FORWARD", fn, i, (int)mode_host[i]);
    for (int k = 0; mode_host[i] >= 0 && k < 3; k++)
      if (!std::isfinite(ref_host[3 * i + k])) return lhw_fail(LHW_ERR_ARG, "%s: ref[%d][%d] = %g is not finite", fn, i, k, ref_host[3 * i + k]);
  }
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  if (humanoid_pin_commands(e->hum, first, count, mode_host, ref_host)) return lhw_fail(LHW_ERR_HIP, "%s: upload failed", fn);
  return LHW_OK;
}

extern "C" int lhw_env_get_pinned_commands(LhwEnv* e, int32_t* mode_host, double* ref_host) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  if (const int rc = commands_supported(e, "lhw_env_get_pinned_commands", true)) return rc;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  humanoid_get_pinned_commands(e->hum, mode_host, ref_host);
  return LHW_OK;
}

// the stepping task's pin (a walk mode and its footstep plan) exists for jvrc_step alone
static int step_pins_supported(const LhwEnv* e, const char* fn) {
  if (!e->hum || e->task != LHW_TASK_JVRC_STEP)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "%s: footstep plans are the command of the stepping task (jvrc_step); this env has none to pin", fn);
  return LHW_OK;
}

extern "C" int lhw_env_pin_step_plans(LhwEnv* e, int32_t first, int32_t count, const LhwStepPin* pins) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  const char* fn = "lhw_env_pin_step_plans";
  if (const int rc = step_pins_supported(e, fn)) return rc;
  if (first < 0 || count < 0 || (int64_t)first + count > e->n_envs)
    return lhw_fail(LHW_ERR_ARG, "%s: envs [first = %d, first + count = %lld) lie outside the batch of %d", fn, (int)first, (long long)first + count, e->n_envs);
  if (count > 0 && !pins) return lhw_fail(LHW_ERR_ARG, "%s: null pins array", fn);
  const int nplans = humanoid_step_nplans(e->hum);
  for (int i = 0; i < count; i++) {
    const LhwStepPin& s = pins[i];
    if (s.reserved != 0) return lhw_fail(LHW_ERR_ARG, "%s: reserved[%d] = %d, must be 0", fn, i, (int)s.reserved);
    if (s.mode < -1 || s.mode > 4)
      return lhw_fail(LHW_ERR_ARG, "%s: mode[%d] = %d, must be -1 (free), 0 CURVED, 1 STANDING, 2 BACKWARD, 3 LATERAL or 4 FORWARD", fn, i, (int)s.mode);
    if (s.mode < 0) continue;   // (a free env: nothing else of the row is read)
    const int nchoice = s.mode == 0 ? nplans : (s.mode == 3 ? 2 : 0);
    if (s.choice < -1 || s.choice >= nchoice) {
      if (!nchoice) return lhw_fail(LHW_ERR_ARG, "%s: choice[%d] = %d, must be -1: mode %d has no choice to pin", fn, i, (int)s.choice, (int)s.mode);
      return lhw_fail(LHW_ERR_ARG, "%s: choice[%d] = %d, must be -1 (drawn) or in [0, %d) for mode %d", fn, i, (int)s.choice, nchoice, (int)s.mode);
    }
    if (s.nseq != 0 && (s.nseq < 2 || s.nseq > LHW_STEP_MAX_SEQ))
      return lhw_fail(LHW_ERR_ARG, "%s: nseq[%d] = %d, must be 0 (generated) or 2 .. %d steps", fn, i, (int)s.nseq, LHW_STEP_MAX_SEQ);
    for (int k = 0; k < s.nseq; k++)
      for (int a = 0; a < 4; a++)
        if (!std::isfinite(s.steps[k][a])) return lhw_fail(LHW_ERR_ARG, "%s: steps[%d][%d][%d] = %g is not finite", fn, i, k, a, s.steps[k][a]);
    if (std::isinf(s.height)) return lhw_fail(LHW_ERR_ARG, "%s: height[%d] = %g, must be finite, or NaN for the schedule's", fn, i, s.height);
  }
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  if (humanoid_pin_step_plans(e->hum, first, count, pins)) return lhw_fail(LHW_ERR_HIP, "%s: upload failed", fn);
  return LHW_OK;
}

extern "C" int lhw_env_get_pinned_step_plans(LhwEnv* e, LhwStepPin* out_host) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  const char* fn = "lhw_env_get_pinned_step_plans";
  if (const int rc = step_pins_supported(e, fn)) return rc;
  if (!out_host) return lhw_fail(LHW_ERR_ARG, "%s: null output array", fn);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  humanoid_get_pinned_step_plans(e->hum, out_host);
  return LHW_OK;
}

extern "C" int lhw_env_pop_episode_stats(LhwEnv* e, double* ret_sum, double* len_sum, int64_t* count) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  double h[3];
  if (const int rc = pop_stats(e, 0, 3, h)) return rc;
  if (ret_sum) *ret_sum = h[0];
  if (len_sum) *len_sum = h[1];
  if (count) *count = (int64_t)h[2];
  return LHW_OK;
}

// the term-statistics block as this env's kernels see it (NULL while the export is off)
static double* term_stats_block(LhwEnv* e) { return e->task == LHW_TASK_CARTPOLE ? e->cps.tstat : humanoid_term_stats(e->hum); }
static int set_term_stats_block(LhwEnv* e, double* block) {
  if (e->task == LHW_TASK_CARTPOLE) { e->cps.tstat = block; return LHW_OK; }
  const int rc = humanoid_set_term_stats(e->hum, block);
  if (rc == -2)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_enable_term_stats: a diagnostic clock of this env is armed (lhw_env_phase_cycles / lhw_env_debug_wave_cycles) and "
                                         "the kernels that keep the statistics carry no clocks");
  return rc ? lhw_fail(LHW_ERR_HIP, "term statistics: parameter upload failed") : LHW_OK;
}

extern "C" int lhw_env_enable_term_stats(LhwEnv* e, int enable) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  if (!enable) return set_term_stats_block(e, nullptr);   // (the block is released with the env)
  const size_t n = (size_t)e->n_envs * (LHW_MAX_REWARD_TERMS + LHW_TS_FIN_STRIDE);
  if (!e->tstat && !(e->tstat = e->mem.get_lazy<double>(n))) return lhw_fail(LHW_ERR_HIP, "term statistics allocation failed (n_envs=%d)", e->n_envs);
  HIPCHK(hipMemset(e->tstat, 0, sizeof(double) * n));
  return set_term_stats_block(e, e->tstat);
}

extern "C" int lhw_env_pop_term_stats(LhwEnv* e, double* term_sum, int64_t* episodes, int64_t* terminated, int64_t* truncated) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  HIPCHK(hipSetDevice(e->device));
  double* dev = term_stats_block(e);
  if (!dev) return lhw_fail(LHW_ERR_ARG, "lhw_env_pop_term_stats: call lhw_env_enable_term_stats(env, 1) first");
  // the finished-episode rows come to the host (96 bytes per env), are added up in env order, and are cleared on the device; the running
  // sums are not touched
  double* fin = dev + (size_t)e->n_envs * LHW_MAX_REWARD_TERMS;
  std::vector<double> rows((size_t)e->n_envs * LHW_TS_FIN_STRIDE);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(rows.data(), fin, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(fin, 0, sizeof(double) * rows.size()));
  double sum[LHW_TS_FIN_STRIDE] = {0};
  for (int n = 0; n < e->n_envs; n++)
    for (int k = 0; k < LHW_TS_FIN_STRIDE; k++) sum[k] += rows[(size_t)n * LHW_TS_FIN_STRIDE + k];
  const int64_t te = (int64_t)sum[LHW_TS_TERMINATED], tr = (int64_t)sum[LHW_TS_TRUNCATED];
  for (int k = 0; term_sum && k < e->n_terms; k++) term_sum[k] = sum[k];
  if (terminated) *terminated = te;
  if (truncated) *truncated = tr;
  if (episodes) *episodes = te + tr;
  return LHW_OK;
}

/* resident workgroups (= waves) per CU the runtime grants the wave-per-env step kernel */
extern "C" int lhw_debug_stepper_occupancy(void) { return humanoid_occupancy(); }

extern "C" int lhw_env_phase_cycles(LhwEnv* e, int enable, int64_t* out16) {
  if (!e || !e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "phase profiling exists for the wave-per-env stepper only");
  HIPCHK(hipSetDevice(e->device));
  static_assert(sizeof(long long) == sizeof(int64_t), "");
  const int rc = humanoid_profile(e->hum, enable, (long long*)out16);
  if (rc == -2) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_phase_cycles: the term statistics are on and their kernels carry no clocks: lhw_env_enable_term_stats(env, 0) first");
  if (rc == -3) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_phase_cycles: the actuator randomisation is armed and its kernels carry no clocks: switch it off first (lhw_env_set_actuator_randomization)");
  if (rc) return lhw_fail(LHW_ERR_HIP, "profile buffer");
  return LHW_OK;
}

/* Diagnostic: first call arms the recording; later calls return, per env, the shader-clock cycles its wavefront group spent
 * in the most recent control-step launch (host pointer [N] int64, synchronous). */
extern "C" int lhw_env_debug_wave_cycles(LhwEnv* e, int64_t* out) {
  if (!e || !e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "wave cycles exist for the humanoid steppers only");
  HIPCHK(hipSetDevice(e->device));
  const int rc = humanoid_wave_cycles(e->hum, (long long*)out);
  if (rc == -2) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_debug_wave_cycles: the term statistics are on and their kernels carry no clocks: lhw_env_enable_term_stats(env, 0) first");
  if (rc == -3) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_env_debug_wave_cycles: the actuator randomisation is armed and its kernels carry no clocks: switch it off first (lhw_env_set_actuator_randomization)");
  if (rc) return lhw_fail(LHW_ERR_HIP, "wave cycle buffer");
  return LHW_OK;
}


extern "C" int lhw_env_pop_fault_stats(LhwEnv* e, int64_t* contact_overflow, int64_t* diverged) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  if (contact_overflow) *contact_overflow = 0;
  if (diverged) *diverged = 0;
  if (!e->hum) return LHW_OK;  // the cartpole kernel has neither contacts nor a divergence path
  double h[2];
  if (const int rc = pop_stats(e, 3, 2, h)) return rc;
  if (contact_overflow) *contact_overflow = (int64_t)h[0];
  if (diverged) *diverged = (int64_t)h[1];
  return LHW_OK;
}

extern "C" int lhw_env_enable_task_inputs(LhwEnv* e, int enable) {
  if (!e || !e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "task inputs exist for the humanoid tasks only");
  HIPCHK(hipSetDevice(e->device));
  if (humanoid_task_inputs(e->hum, false, enable ? 1 : 0, nullptr, nullptr)) return lhw_fail(LHW_ERR_HIP, "task input buffer");
  return LHW_OK;
}
extern "C" int lhw_env_get_task_inputs(LhwEnv* e, double* out_host) {
  if (!e || !e->hum || !out_host) return lhw_fail(LHW_ERR_ARG, "null argument / not a humanoid task");
  HIPCHK(hipSetDevice(e->device));
  const int rc = humanoid_task_inputs(e->hum, false, -1, out_host, nullptr);
  if (rc == -2) return lhw_fail(LHW_ERR_ARG, "lhw_env_get_task_inputs: call lhw_env_enable_task_inputs(env, 1) first");
  if (rc) return lhw_fail(LHW_ERR_HIP, "task input copy");
  return LHW_OK;
}
extern "C" int lhw_env_task_inputs_device(LhwEnv* e, double** out_dev) {
  if (!e || !e->hum || !out_dev) return lhw_fail(LHW_ERR_ARG, "null argument / not a humanoid task");
  return humanoid_task_inputs(e->hum, false, -1, nullptr, out_dev) ? lhw_fail(LHW_ERR_HIP, "task input buffer") : LHW_OK;
}
extern "C" int lhw_env_enable_step_task_inputs(LhwEnv* e, int enable) {
  if (!e || !e->hum || e->task != LHW_TASK_JVRC_STEP) return lhw_fail(LHW_ERR_UNSUPPORTED, "the stepping task-input record exists for the stepping task only");
  HIPCHK(hipSetDevice(e->device));
  if (humanoid_task_inputs(e->hum, true, enable ? 1 : 0, nullptr, nullptr)) return lhw_fail(LHW_ERR_HIP, "stepping task input buffer");
  return LHW_OK;
}
extern "C" int lhw_env_get_step_task_inputs(LhwEnv* e, double* out_host) {
  if (!e || !e->hum || e->task != LHW_TASK_JVRC_STEP || !out_host) return lhw_fail(LHW_ERR_ARG, "null argument / not a stepping-task env");
  HIPCHK(hipSetDevice(e->device));
  const int rc = humanoid_task_inputs(e->hum, true, -1, out_host, nullptr);
  if (rc == -2) return lhw_fail(LHW_ERR_ARG, "lhw_env_get_step_task_inputs: call lhw_env_enable_step_task_inputs(env, 1) first");
  if (rc) return lhw_fail(LHW_ERR_HIP, "stepping task input copy");
  return LHW_OK;
}
extern "C" int lhw_env_step_task_inputs_device(LhwEnv* e, double** out_dev) {
  if (!e || !e->hum || e->task != LHW_TASK_JVRC_STEP || !out_dev) return lhw_fail(LHW_ERR_ARG, "null argument / not a stepping-task env");
  return humanoid_task_inputs(e->hum, true, -1, nullptr, out_dev) ? lhw_fail(LHW_ERR_HIP, "stepping task input buffer") : LHW_OK;
}
extern "C" int lhw_env_get_actuator_state(LhwEnv* e, double* pos_host, double* vel_host, double* torque_host) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  if (!e->hum) return lhw_fail(LHW_ERR_UNSUPPORTED, "actuator state is kept by the humanoid steppers only");
  HIPCHK(hipSetDevice(e->device));
  if (humanoid_actuator_state(e->hum, pos_host, vel_host, torque_host)) return lhw_fail(LHW_ERR_HIP, "actuator state copy failed");
  return LHW_OK;
}

extern "C" int lhw_env_pop_rerun_count(LhwEnv* e, int64_t* reruns) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  if (reruns) *reruns = 0;
  if (!e->hum) return LHW_OK;
  double h = 0;
  if (const int rc = pop_stats(e, 5, 1, &h)) return rc;
  if (reruns) *reruns = (int64_t)h;
  return LHW_OK;
}

extern "C" int lhw_env_debug_step_record(LhwEnv* e, double* seq, double* floor_z, int32_t* istate) {
  if (!e || !e->hum || e->task != LHW_TASK_JVRC_STEP) return lhw_fail(LHW_ERR_ARG, "step record: not a stepping-task env");
  if (humanoid_step_record(e->hum, seq, floor_z, istate)) return lhw_fail(LHW_ERR_HIP, "step record copy failed");
  return LHW_OK;
}

extern "C" int lhw_env_set_iteration(LhwEnv* e, int64_t iteration) {
  if (!e) return lhw_fail(LHW_ERR_ARG, "null env");
  if (e->hum) humanoid_set_iteration(e->hum, iteration);
  return LHW_OK;
}
