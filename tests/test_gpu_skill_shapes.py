"""zenv_collect_skill's two kernels (csrc/skill_collect.hip) at their edges: k_skill_inverse_f32 with S = 1, 2 and 32
(kMaxSkills: EB * S = 128 logit threads), h = 1, 64 and 191, ragged workgroups (N = 1, 3, 5, 4097), workgroups whose
four envs are all done next to mixed ones, inverse weights at scale 3 (logits beyond exp's float32 range, where the
log-sum-exp shift matters), prior logits spanning +-30 and diversity_coef = 0 with an inverse model loaded;
k_skill_hi_gae with L = 1 (every frame a window) and T = L (W = 1: only the bootstrap), lambda 0 and 1.  The diversity
against the float64 InverseModel (tests/skill_collect_ref.py with dtype=float64), the low-level reward bit for bit,
the high level's reward, mask, advantage and return against float64 (tests/collect_ref.gae with no discount)."""
import numpy as np
import pytest
import torch

from tests import collect_ref, skill_ref
from tests.skill_collect_ref import inverse_log_softmax, random_inverse_state_dict

pytestmark = pytest.mark.gpu

F64 = torch.float64
TSP, TTSP, CM = 0, 1, 2
# diversity: |dev - ref64| <= DIV_TOL max(1, |ref64|), or at weight scale > 1 (logits in the hundreds, where torch's own
# float32 result is no longer within that of float64) K_F32 |ref32 - ref64| -- as test_gpu_hier_shapes.py holds the
# skill logits.  Measured: 9.6e-7 relative at scale 1, 4.8e-6 at scale 3.  A wrong skill, frame or a log-sum-exp
# without its shift is off by O(1) or not finite.
DIV_TOL, K_F32 = 1e-5, 16.0
# the high level's window sum and GAE: within HI_U units of 2^-24 times the float64 magnitude (measured 1.3)
HI_U = 4.0
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("skill shapes worst: %-40s %.4g" % (k, WORST[k]))


def _inverse_logits64(sd, obs, zone_obs):
    """InverseModel's logits before the log-softmax, float64 (to show that they leave exp's float32 range)."""
    sd = {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items()}
    o = torch.as_tensor(np.asarray(obs, np.float64))
    zo = torch.as_tensor(np.asarray(zone_obs, np.float64))
    bs, nz = zo.shape[0], zo.shape[1]
    x = torch.cat([o.view(bs, 1, 8).expand(bs, nz, 8), zo], dim=-1)
    y = torch.relu(x @ sd["zone_net.0.weight"].T + sd["zone_net.0.bias"])
    y = torch.relu(y @ sd["zone_net.2.weight"].T + sd["zone_net.2.bias"])
    y = (y @ sd["zone_net.4.weight"].T + sd["zone_net.4.bias"]).sum(dim=1) / nz
    c = torch.relu(torch.cat([o, y], dim=-1) @ sd["combine_net.0.weight"].T + sd["combine_net.0.bias"])
    return (c @ sd["combine_net.2.weight"].T + sd["combine_net.2.bias"]).numpy()


def _env(Z, task, zones, n, seed, num_steps):
    keep = {25: 0.40, 15: 0.55}.get(zones, 0.45)
    env = Z.ZoneVecEnv(Z.default_config(task, zones, zones_keepout=keep, num_steps=num_steps), n)
    env.build_bank(seed, n)
    env.schedule_sequential()
    env.reset()
    return env


def _raw(Z, env, T, L):
    lo_l, _ = Z.skill_experience_layout(env.num_envs, env.num_zones, env.zone_feat, T, L)
    out = {}
    for name, (f, s, dt) in lo_l.items():
        a = np.empty(s, dt)
        Z._native.check(Z._native.lib().zenv_get(env._h, f, a.ctypes.data, 0))
        out[name] = a
    return out


def _check_call(Z, env, inv_sd, prior, coef, T, L, lam, scale, carried, tag, want_done=None):
    """One collect_skills call on env, checked against float64.  Returns (1 - done of the last frame, done [T, N])."""
    n, S = env.num_envs, len(prior)
    lo, hi, _, _ = env.collect_skills(T, policy_seed=5, discount=0.99, gae_lambda=lam, diversity_coef=coef,
                                      skill_prior_logits=prior)
    raw = _raw(Z, env, T, L)
    o_T, zo_T = env.observations()
    W = T // L
    mask = raw["mask"]
    assert np.array_equal(mask[0], carried), tag
    done = np.concatenate([1 - mask[1:], env.get(Z._native.F_DONE).astype(np.float32)[None]]).astype(bool)
    if want_done is not None:
        assert np.array_equal(done[want_done[0]], want_done[1]), tag
    # the diversity: float64 InverseModel on obs_{t+1}, minus the float64 log-softmax of the prior, 0 where done_t
    obs_n = np.concatenate([raw["obs"][1:], o_T[None]]).reshape(T * n, 8)
    zo_n = np.concatenate([raw["zone_obs"][1:], zo_T[None]]).reshape(T * n, env.num_zones, env.zone_feat)
    l64 = inverse_log_softmax(inv_sd, obs_n, zo_n, dtype=F64)
    l32 = inverse_log_softmax(inv_sd, obs_n, zo_n).astype(np.float64)
    p = np.asarray(prior, np.float64)
    p64 = p - p.max() - np.log(np.exp(p - p.max()).sum())
    sk = raw["skill"].reshape(-1)
    assert ((sk >= 0) & (sk < S)).all()
    live = ~done.reshape(-1)
    want = np.where(live, l64[np.arange(T * n), sk] - p64[sk], 0.0)
    d32 = np.abs(l32[np.arange(T * n), sk] - l64[np.arange(T * n), sk])
    dev = raw["diversity"].reshape(-1).astype(np.float64)
    assert (dev[~live] == 0).all() and not np.signbit(dev[~live]).any(), tag     # a finished env: exactly +0
    err = np.abs(dev - want)[live]
    rel = err / np.maximum(1.0, np.abs(want[live]))
    _note("diversity rel (scale %g)" % scale, rel.max(initial=0))
    bar = np.maximum(DIV_TOL * np.maximum(1.0, np.abs(want[live])), K_F32 * d32[live] if scale > 1 else 0)
    assert (err <= bar).all(), (tag, float(err.max(initial=0)))
    # the low-level reward: env_reward + coef * diversity, two float32 roundings
    f = np.float32
    lo_r = (raw["env_reward"] + (f(coef) * raw["diversity"]).astype(f)).astype(f)
    assert np.array_equal(raw["reward"].view(np.uint32), lo_r.view(np.uint32)), tag
    # the high level: window sums, next_mask, GAE with no discount (collect_ref.gae with discount 1)
    er = raw["env_reward"].astype(np.float64).reshape(W, L, n)
    r64, rmag = er.sum(1), np.abs(er).sum(1)
    hr = hi["reward"].reshape(n, W).T
    u = np.abs(hr - r64) / np.maximum(rmag * 2.0 ** -24, 1e-30)
    _note("hi reward units", u.max())
    assert u.max() <= HI_U, tag
    last = 1.0 - done[-1].astype(np.float32)
    hm = np.concatenate([mask[0][None], mask[L::L]]) if W > 1 else mask[:1]
    want_m = np.concatenate([hm[1:], last[None]])
    assert np.array_equal(hi["mask"].reshape(n, W).T, want_m), tag
    hv = hi["value"].reshape(n, W).T
    adv, ret, gmag = collect_ref.gae(hr, hv, hm, last, env.get(Z._native.F_SKILL_VALUE), 1.0, np.float32(lam))
    for name, devv, w in (("advantage", hi["advantage"], adv), ("returnn", hi["returnn"], ret)):
        u = np.abs(devv.reshape(n, W).T - w) / np.maximum((gmag + np.abs(hv)) * 2.0 ** -24, 1e-30)
        _note("hi %s units (lambda %g)" % (name, lam), u.max())
        assert u.max() <= HI_U, (tag, name, float(u.max()))
    return last, done


# (task, Z, S, h, N, L, T, weight scale, prior spread, coef, lambda, num_steps)
SHAPES = [
    (TSP, 3, 1, 1, 1, 1, 3, 1.0, 0.0, 0.5, 0.95, 2),          # S = 1, h = 1, N = 1, L = 1
    (TTSP, 5, 2, 64, 3, 4, 4, 3.0, 30.0, 0.5, 1.0, 3),       # T = L (W = 1), prior +-30, scale 3
    (CM, 6, 32, 191, 5, 2, 6, 3.0, 30.0, 0.25, 0.0, 5),      # S = kMaxSkills, h = 191, ragged
    (TSP, 9, 32, 64, 4097, 3, 6, 1.0, 2.0, 0.0, 0.95, 4),    # diversity_coef = 0 with an inverse model
]


@pytest.mark.parametrize("shape", SHAPES, ids=["S%d_h%d_N%d_L%d_T%d" % (s[2], s[3], s[4], s[5], s[6]) for s in SHAPES])
def test_collect_skill_edge_shapes(zenv_mod, shape):
    Z = zenv_mod
    task, zones, S, h, n, L, T, scale, spread, coef, lam, num_steps = shape
    env = _env(Z, task, zones, n, 13, num_steps)
    hi, lo = skill_ref.random_state_dicts(env.zone_feat, S, h=h, seed=3)
    env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo), skill_len=L)
    inv = random_inverse_state_dict(env.zone_feat, S, h=h, seed=4, weight_scale=scale)
    env.load_skill_inverse(Z.inverse_tensors_from_state_dict(inv, S))
    prior = (np.linspace(-spread, spread, S) if S > 1 else np.zeros(1)).astype(np.float32)
    carried = np.ones(n, np.float32)
    ended = 0
    for c in range(2):
        carried, done = _check_call(Z, env, inv, prior, coef, T, L, lam, scale, carried, (shape, c))
        ended += int(done.sum())
    assert ended > 0, "no episode ended"
    if S == 32 and scale > 1:                      # the shift is needed: exp of the largest logit overflows float32
        o, zo = env.observations()
        assert np.abs(_inverse_logits64(inv, o, zo)).max() > 89
    env.close()


def test_collect_skill_all_done_workgroups(zenv_mod):
    """Workgroup w (envs 4w .. 4w+3) has (w % 5) envs left running, the others ended by a NaN action without a reset:
    a call leaves their frames of the first window done -- diversity exactly 0, lo reward = env reward (0) -- and a
    workgroup with none left running takes the skip branch over slots an earlier call of the same T had filled."""
    Z = zenv_mod
    n, S, L, T = 203, 4, 4, 8
    env = _env(Z, TSP, 25, n, 17, 40)
    hi, lo = skill_ref.random_state_dicts(env.zone_feat, S, h=64, seed=5)
    env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo), skill_len=L)
    inv = random_inverse_state_dict(env.zone_feat, S, h=64, seed=6)
    env.load_skill_inverse(Z.inverse_tensors_from_state_dict(inv, S))
    prior = np.array([0.5, -1.0, 2.0, 0.0], np.float32)
    carried, _ = _check_call(Z, env, inv, prior, 0.5, T, L, 0.95, 1.0, np.ones(n, np.float32), "fill")
    first = _raw(Z, env, T, L)
    assert (first["diversity"][:L - 1] != 0).all()          # the slots the skip branch must overwrite
    i = np.arange(n)
    running = (i % 4) < ((i // 4) % 5)
    a = np.zeros((n, 2), np.float32)
    a[~running, 0] = np.nan
    env.step(a, auto_reset=False)
    # self.mask is the collector's: the NaN step leaves it, the next call's frame 0 records the first call's last frame
    _, done = _check_call(Z, env, inv, prior, 0.5, T, L, 0.95, 1.0, carried, "pattern",
                          want_done=(slice(0, L - 1), np.broadcast_to(~running, (L - 1, n))))
    full = np.array([done[:L - 1, 4 * w:4 * w + 4].all() for w in range((n + 3) // 4)])
    assert full.sum() >= 5 and (~full).sum() >= 5
    env.close()
