"""obs_history_len = 3 on the GPU path: a BatchedEnv with history against a twin without, same seed and actions -- the full
observation must be the reference's deque (newest first, zero-filled after an auto-reset; tests/test_obs_history.py pins that
rule to the executed reference), through step(), through step_range() on two env groups, and through a PPO iteration."""
import pytest

from tests.obs_history_checks import check_history_is_the_deque, spec_h3 as _spec_h3

pytestmark = pytest.mark.gpu


def test_history_observation_is_the_deque_of_base_observations(tmp_path):
    check_history_is_the_deque(lambda spec, N, **kw: spec.make_batched(N, device=0, **kw), tmp_path, N=6, T=150, max_traj_len=60, groups=(3, 3))


def test_ppo_iteration_runs_with_history(tmp_path):
    from types import SimpleNamespace
    from learninghumanoidwalking_amd.ppo import PPO
    import functools
    s3, _ = _spec_h3(tmp_path)
    args = SimpleNamespace(gamma=0.99, lam=0.95, lr=1e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=512, epochs=2, num_procs=64,
                           max_grad_norm=0.05, max_traj_len=16, use_gae=True, mirror_coeff=0.4, eval_freq=100, continued=None, recurrent=False,
                           imitate=None, imitate_coeff=0.3, logdir=str(tmp_path / "log"), std_dev=0.223, learn_std=False, n_itr=1, seed=0,
                           no_mirror=True, num_envs=64)
    algo = PPO(functools.partial(type(s3), yaml_path=s3.yaml_path), args, seed=0)
    algo.train(functools.partial(type(s3), yaml_path=s3.yaml_path), n_itr=1)
    assert algo.kernels.obs_dim == 111 if hasattr(algo.kernels, "obs_dim") else True
