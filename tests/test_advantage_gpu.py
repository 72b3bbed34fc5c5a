"""The advantage kernels at the benchmark's shapes and at small n: lhw_gae against a float64 reverse scan, lhw_moments +
lhw_standardize (through the path of PPO._normalize_advantages) against float64 numpy."""
import numpy as np
import pytest
import torch

GAMMA, LAM = 0.99, 0.95


def _gae_scan(rew, val, done, vterm, vfinal, gamma, lam):
    """float64 GAE(lambda) over a time-major [T][N] rollout, all envs at once, with the bootstrap rules of oracle.ppo_oracle.gae_batch:
    a done flag ends the trajectory at t (bit 0 set: terminal, no bootstrap; otherwise bootstrap from vterm), the last step of a
    column that does not end bootstraps from vfinal."""
    T, N = rew.shape
    ret = np.zeros((T, N))
    gae, nextv = np.zeros(N), vfinal.astype(np.float64)
    for t in range(T - 1, -1, -1):
        d = done[t] != 0
        nextv = np.where(d, np.where(done[t] & 1, 0.0, vterm[t].astype(np.float64)), nextv)
        gae = np.where(d, 0.0, gae)
        v = val[t].astype(np.float64)
        gae = rew[t] + gamma * nextv - v + gamma * lam * gae
        ret[t] = gae + v
        nextv = v
    return ret


def _rollout(rs, T, N, p_done=0.05):
    rew = (rs.normal(size=(T, N)) * 0.5).astype(np.float32)
    val = rs.normal(size=(T, N)).astype(np.float32)
    # every flag value 0..3 (bit 0: terminal, bit 1: time limit)
    done = np.where(rs.uniform(size=(T, N)) < p_done, rs.integers(1, 4, size=(T, N)), 0).astype(np.uint8)
    vterm = rs.normal(size=(T, N)).astype(np.float32)
    vfinal = rs.normal(size=N).astype(np.float32)
    return rew, val, done, vterm, vfinal


def test_vectorised_scan_matches_the_oracle():
    """The reference of the GPU test below, against the oracle's per-env loop (CPU only; the oracle is far too slow at 400 x 4097)."""
    from oracle import ppo_oracle as po
    rs = np.random.default_rng(0)
    rew, val, done, vterm, vfinal = _rollout(rs, 37, 11, p_done=0.15)
    assert set(np.unique(done)) == {0, 1, 2, 3}
    np.testing.assert_allclose(_gae_scan(rew, val, done, vterm, vfinal, GAMMA, LAM), po.gae_batch(rew, val, done, vterm, vfinal, GAMMA, LAM),
                               rtol=0, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(400, 4097), (37, 513), (1, 256)])
def test_gae_matches_float64_scan(T, N):
    """Several blocks and a ragged last block (N = 4097, 513), the benchmark's T = 400, and T = 1 (a single step: only the bootstrap)."""
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels
    k = PpoKernels(5, 1, hidden=64, max_rows=64)
    rs = np.random.default_rng(T + N)
    rew, val, done, vterm, vfinal = _rollout(rs, T, N)
    if T == 1:
        done[0, :4] = [0, 1, 2, 3]
    assert set(np.unique(done)) == {0, 1, 2, 3}
    ref = _gae_scan(rew, val, done, vterm, vfinal, GAMMA, LAM)
    # the bar is the existing 1e-6 absolute (float64 scan, float32 store): it holds only while |returns| < 16, where half a float32
    # ulp is < 1e-6
    assert np.abs(ref).max() < 16
    c = lambda a: torch.from_numpy(a).cuda()
    ret, adv = k.gae(c(rew), c(val), c(done), c(vterm), c(vfinal), GAMMA, LAM)
    np.testing.assert_allclose(ret.cpu().numpy(), ref, rtol=0, atol=1e-6)
    np.testing.assert_allclose(adv.cpu().numpy(), ref - val, rtol=0, atol=1e-6)     # returns.float() - values.float() (ppo.py:484)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 17, 255, 257, 65537, 400 * 4096])
@pytest.mark.parametrize("offset", [100.0, 0.0])
def test_advantage_standardisation_matches_float64(n, offset):
    """PPO._normalize_advantages' device path: lhw_moments -> dist_utils.global_moments_pack -> lhw_standardize.  Small n tells an
    unbiased std from a biased one (sqrt(2) apart at n = 2) and a count that is off by one; offset-mean data tests the cancellation in
    sum of squares - n mean^2."""
    from learninghumanoidwalking_amd import dist_utils
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels
    eps = 1e-5
    k = PpoKernels(5, 1, hidden=64, max_rows=64)
    rs = np.random.default_rng(n)
    x = (offset + rs.normal(size=n)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    pack = dist_utils.global_moments_pack(k.moments(xd), xd.numel())
    x64 = x.astype(np.float64)
    p = pack.cpu().numpy()
    # float64 sums of float32 inputs in another order: relative error ~ log2(n) * 2^-53, far below 1e-12 (of the sum of |x|)
    assert abs(p[0] - x64.sum()) <= 1e-12 * np.abs(x64).sum(), (p[0], x64.sum())
    assert abs(p[1] - (x64 * x64).sum()) <= 1e-12 * (x64 * x64).sum(), (p[1], (x64 * x64).sum())
    assert p[2] == n
    k.standardize(xd, pack, eps)
    out = xd.cpu().numpy().astype(np.float64)
    mean, std = x64.mean(), x64.std(ddof=1)
    z = (x64 - mean) / (std + eps)
    # the kernel rounds the mean and 1 / (std + eps) to float32 (as the float32 tensors of ppo.py:484-485 hold them), then
    # (x - mean) * inv in float32: |error| <= half an ulp of the mean times inv (x - mean itself is exact when x and the mean are within
    # a factor of 2, else a half ulp of the difference), plus 2^-24 relative from inv and 2^-24 from the product
    inv = 1.0 / (std + eps)
    tol = (0.5 * np.spacing(np.float32(abs(mean))) + 0.5 * np.spacing(np.abs(x64 - mean).astype(np.float32))) * inv \
        + 3 * 2.0 ** -24 * np.abs(z) + 1e-30
    err = np.abs(out - z)
    assert (err <= tol).all(), f"n={n}: worst {float((err / tol).max()):.3g} x the bar at {int((err / tol).argmax())}"
    if n <= 257:
        # the bar can tell a biased std (or a count off by one) from the right one
        zb = (x64 - mean) / (x64.std(ddof=0) + eps)
        assert (np.abs(out - zb) > 10 * tol).any()
