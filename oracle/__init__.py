"""CPU oracle -- TEST INFRASTRUCTURE ONLY (see oracle/mjc_oracle.c header).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package.
"""


def make_oracle_env(name, seed=0, env_id=0, max_traj_len=400):
    """(env, obs_dim, act_dim) for the CPU baseline / parity harnesses."""
    from importlib import import_module
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    spec_cls = ENVIRONMENTS[name]
    if name == "cartpole":
        from .env_cartpole import OracleCartpoleEnv
        spec = spec_cls()
        env = OracleCartpoleEnv(spec.model(), seed=seed, env_id=env_id, kp=spec.kp, kd=spec.kd, frame_skip=spec.frame_skip, max_traj_len=max_traj_len)
    else:       # oracle/env_<name>.py: make_oracle_<name>
        env = getattr(import_module(f".env_{name}", __name__), f"make_oracle_{name}")(seed=seed, env_id=env_id, max_traj_len=max_traj_len)
    return env, spec_cls.base_obs_dim, spec_cls.act_dim
