"""TEST INFRASTRUCTURE -- numpy restatement of the device's random draws (checker only).

Every draw of the device policies is keyed by Philox4x32-10 (mlp_head_out.hpp, include/zenv.h): counter
{g_lo, g_hi, step_index, tag}, key (seed_lo, seed_hi), with g = env_index0 + env (the global env index) and step_index =
zenv_step_count of the call.  One stream per tag:
* 0x4D4C50 -- the action noise: Box-Muller on the uniforms of c[0] and c[1] (the flat and both low-level networks)
* 0x48474C -- the Zone-goals goal draw: the uniform of c[0]
* 0x534B4C -- the fixed-length-skills skill draw: the uniform of c[0]
A uniform is ((x >> 8) + 0.5) * 2^-24, evaluated in float32 as the device does: for x >> 8 >= 2^23 the + 0.5 rounds (to
even), so the top value is exactly 1.0, not 1 - 2^-25.
"""
import numpy as np

TAG_ACTION, TAG_GOAL, TAG_SKILL = 0x4D4C50, 0x48474C, 0x534B4C
_M0, _M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 words (scalars or arrays of one shape), key: 2 words -> 4 uint32 arrays."""
    c = [np.asarray(x, np.uint64) & _MASK for x in ctr]
    k0, k1 = (np.asarray(x, np.uint64) & _MASK for x in key)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(_MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(_MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(_W0)) & np.uint64(_MASK)
        k1 = (k1 + np.uint64(_W1)) & np.uint64(_MASK)
    return [x.astype(np.uint32) for x in c]


def uniform(x):
    """uint32 -> float32 in (0, 1]: ((x >> 8) + 0.5) * 2^-24 in float32 arithmetic."""
    hi = (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32)
    return ((hi + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float32)


def _draw(n, seed, env_index0, step_index, tag):
    g = np.uint64(env_index0) + np.arange(n, dtype=np.uint64)
    seed = int(seed)
    ctr = (g & np.uint64(_MASK), g >> np.uint64(32), np.full(n, int(step_index) & _MASK, np.uint64),
           np.full(n, tag, np.uint64))
    return philox4x32_10(ctr, (seed & _MASK, (seed >> 32) & _MASK))


def goal_uniform(n, seed, env_index0, step_index):
    """float32 [n]: the uniform of the goal draw of envs 0 .. n-1."""
    return uniform(_draw(n, seed, env_index0, step_index, TAG_GOAL)[0])


def skill_uniform(n, seed, env_index0, step_index):
    """float32 [n]: the uniform of the skill draw of envs 0 .. n-1."""
    return uniform(_draw(n, seed, env_index0, step_index, TAG_SKILL)[0])


def action_noise(n, seed, env_index0, step_index):
    """float64 [n, 2]: the standard normal pair of the action draw, Box-Muller in float64 on the two float32 uniforms.
    The angle is formed as the device forms it, float32(float32(2 pi) * u2): the float32 rounding of that product moves
    the angle by up to 4e-7, which would otherwise dominate a comparison at the level of a few float32 ulps."""
    c = _draw(n, seed, env_index0, step_index, TAG_ACTION)
    u1 = uniform(c[0]).astype(np.float64)
    ang = (np.float32(6.283185307179586) * uniform(c[1])).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
