"""TEST INFRASTRUCTURE -- float64 restatements of what zenv_collect records besides the env frames (checker only),
shared by tests/test_gpu_collect_paths.py and tests/test_collect_ref_cpu.py:
* ``normal_log_prob``: Normal(mu, std).log_prob(action) per action dimension (base.py:160), float64
* ``action_draw``: the device's dist.sample() (mlp_head_out.hpp, mlp_action) in float32 numpy -- Box-Muller on the two
  Philox uniforms of tests/philox_ref.py; ``action_draw_ulps`` measures a recorded action against the float64 draw
* ``gae``: the GAE recursion of base.py:190-196 on time-major [T, N] records, float64 -- advantage and returnn, and the
  magnitude every advantage's float32 rounding error scales with
"""
import numpy as np

from tests import philox_ref

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def normal_log_prob(action, mu, std):
    """float64 [..., 2]: -((a - mu) / std)^2 / 2 - log(std) - log(2 pi) / 2, and the sum of the terms' magnitudes
    (the scale a float32 evaluation's rounding error is relative to)."""
    a, m, s = (np.asarray(x, np.float64) for x in (action, mu, std))
    z = (a - m) / s
    q, ls = 0.5 * z * z, np.log(s)
    return -q - ls - HALF_LOG_2PI, q + np.abs(ls) + HALF_LOG_2PI


def action_draw(mu, std, seed, env_index0, step_index):
    """float32 [n, 2]: mu + std * rad * (cos, sin)(2 pi u2), rad = sqrt(-2 log u1), every operation in float32 as the
    device forms it (mu, std: float32 [n, 2], the kernel's own)."""
    mu, std = np.asarray(mu, np.float32), np.asarray(std, np.float32)
    n = len(mu)
    c = philox_ref._draw(n, seed, env_index0, step_index, philox_ref.TAG_ACTION)
    u1, u2 = philox_ref.uniform(c[0]), philox_ref.uniform(c[1])
    rad = np.sqrt(np.float32(-2.0) * np.log(u1)).astype(np.float32)
    ang = (np.float32(6.283185307179586) * u2).astype(np.float32)
    e = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).astype(np.float32)
    return (mu + std * e).astype(np.float32)


def action_draw_ulps(a, mu, std, seed, env_index0, step_index):
    """|a - (mu + std eps64)| in float32 ulps of |mu| + std |eps64| per element (eps64: philox_ref.action_noise, the
    float64 Box-Muller on the device's uniforms) -- the measure test_mlp_sample_action_draws_exactly holds to 4."""
    eps = philox_ref.action_noise(len(mu), seed, env_index0, step_index)
    mu, std = np.asarray(mu, np.float64), np.asarray(std, np.float64)
    mag = np.abs(mu) + std * np.hypot(eps[:, :1], eps[:, 1:])
    return np.abs(np.asarray(a, np.float64) - (mu + std * eps)) / (mag * 2.0 ** -23)


def gae(reward, value, mask, cur_mask, next_value, discount, gae_lambda):
    """base.py:190-196, float64.  reward / value / mask: time-major [T, N] (mask[i] = 1 - done of frame i - 1);
    cur_mask: self.mask after the frames [N]; next_value: value(obs_T) [N]; discount / gae_lambda: the values the device
    used (pass the float32-rounded ones).  -> (advantage, returnn, magnitude) [T, N]: magnitude_i = |r_i| +
    |discount v_{i+1} m_{i+1}| + |v_i| + discount gae_lambda m_{i+1} magnitude_{i+1}, which bounds the float32
    recursion's error in units of its rounding (|adv - adv64| <= c 2^-24 magnitude, c a few)."""
    r, v, m = (np.asarray(x, np.float64) for x in (reward, value, mask))
    T, N = r.shape
    g, lam = float(discount), float(gae_lambda)
    adv, mag = np.zeros((T, N)), np.zeros((T, N))
    nv, nm = np.asarray(next_value, np.float64), np.asarray(cur_mask, np.float64)
    na, nmag = np.zeros(N), np.zeros(N)
    for i in reversed(range(T)):
        delta = r[i] + g * nv * nm - v[i]
        adv[i] = delta + g * lam * na * nm
        mag[i] = np.abs(r[i]) + np.abs(g * nv * nm) + np.abs(v[i]) + g * lam * nm * nmag
        nv, nm, na, nmag = v[i], m[i], adv[i], mag[i]
    return adv, v + adv, mag
