"""TEST INFRASTRUCTURE -- the numpy restatement of zenv_collect_option's bookkeeping (checker only), shared by
tests/test_option_collect_cpu.py and tests/test_gpu_option_collect.py: `replay` drives a second handle frame by frame
with zenv_policy(OPTION_SAMPLE) + zenv_step and puts back, with zenv_set_skills, the skill of every env whose episode
ended while its option went on (the collector's survival rule expressed with the existing API); `expected_hi` turns
such a record into the high-level rows of every call (options/src/torch_ac/algos/_hier_policy_opt.py:14-108)."""
import numpy as np

LAM, GAMMA = 0.95, 0.99


def replay(Z, env, frames, seed):
    """Drive `env` for `frames` frames; the per-frame record.  pick[t, j]: env j picked its skill at frame t."""
    keys = ("obs", "zone_obs", "pick", "skill", "ended", "pick_value", "logits", "action", "mu", "std", "value",
            "term_mu", "term_std", "term_action", "reward", "done")
    log = {k: [] for k in keys}
    for _ in range(frames):
        o, zo = env.observations()
        before, ended_before = env.get(Z.F_SKILL), env.get(Z.F_OPTION_ENDED)
        env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=seed)
        skill, ended = env.get(Z.F_SKILL), env.get(Z.F_OPTION_ENDED)
        log["obs"].append(o)
        log["zone_obs"].append(zo)
        log["pick"].append(((before < 0) | (ended_before != 0)) & (skill >= 0))
        log["skill"].append(skill)
        log["ended"].append(ended.astype(bool))
        log["pick_value"].append(env.get(Z.F_SKILL_VALUE))
        log["logits"].append(env.get(Z.F_SKILL_LOGITS))
        log["action"].append(env.get(Z.F_ACTIONS))
        log["mu"].append(env.get(Z.F_POLICY_MU))
        log["std"].append(env.get(Z.F_POLICY_STD))
        log["value"].append(env.get(Z.F_POLICY_VALUE))
        log["term_mu"].append(env.get(Z.F_OPTION_TERM_MU))
        log["term_std"].append(env.get(Z.F_OPTION_TERM_STD))
        log["term_action"].append(env.get(Z.F_OPTION_TERM_ACTION))
        env.step(None, auto_reset=True)
        _, _, r, d, _ = env.results()
        log["reward"].append(r)
        log["done"].append(d.astype(bool))
        keep = d.astype(bool) & (ended == 0) & (skill >= 0)      # the episode ended, the option did not
        if keep.any():
            env.set_skills(np.where(keep, skill, -1).astype(np.int32))
    return {k: np.stack(v) for k, v in log.items()}


def expected_age(b, upto=None):
    """ZENV_F_SKILL_AGE after frames 0 .. upto-1: the low-level steps since the env's last pick (auto-resets do not
    restart it).  Every env of `b` must have picked at least once."""
    pick = b["pick"][:upto]
    frames, n = pick.shape
    last = np.where(pick, np.arange(frames)[:, None], -1).max(0)
    assert (last >= 0).all()
    return (frames - last).astype(np.int32)


def expected_hi(b, T, n_calls, v_final, lam=LAM, dtype=np.float32):
    """The numpy restatement: per call, per env, the closed transitions in order with their GAE.  b: pick, ended, done
    (bool [frames, n]), reward, pick_value (float32 [frames, n]), skill (int [frames, n]).  T: frames per call, or a list
    of them; v_final[c] = V_hi(obs_T) after call c; dtype: the arithmetic's.  Also returns how often each boundary case was met:
      span       a row whose pick lies in an earlier call
      mask0 / mask1   rows closed with hi_mask 0 / 1
      bootstrap  a row with hi_mask 1 whose V_next is V_hi(obs_T)
      survived   a row whose option ran across an auto-reset (a done between its pick and its close): the reward sums
                 two episodes
      no_rows    (call, env) pairs without a row"""
    f = dtype                                             # float32: the device's arithmetic; float64 for a float64 record
    n = b["pick"].shape[1]
    starts = np.concatenate([[0], np.cumsum([T] * n_calls if np.isscalar(T) else T)]).astype(int)
    out = [[[] for _ in range(n)] for _ in range(n_calls)]
    seen = {"span": 0, "mask0": 0, "mask1": 0, "bootstrap": 0, "survived": 0, "no_rows": 0}
    lam = f(lam)
    for j in range(n):
        hr = f(0)
        open_t = None
        events = []                                        # (close frame, pick frame, reward, mask)
        picks = []
        for t in range(starts[-1]):
            if b["pick"][t, j]:
                assert open_t is None
                open_t = t
                picks.append(t)
            hr = f(hr + f(b["reward"][t, j]))
            if b["ended"][t, j]:
                if open_t is not None:
                    events.append((t, open_t, hr, 0.0 if b["done"][t, j] else 1.0))
                    open_t = None
                hr = f(0)
        for c in range(n_calls):
            closed = [e for e in events if starts[c] <= e[0] < starts[c + 1]]
            rows = []
            for tc, tp, r, m in closed:
                nxt = [p for p in picks if p > tp]
                if nxt and nxt[0] < starts[c + 1]:
                    vn = b["pick_value"][nxt[0], j]
                else:
                    vn = v_final[c][j]
                    seen["bootstrap"] += m == 1.0
                rows.append(dict(t_pick=tp, t_close=tc, skill=int(b["skill"][tp, j]),
                                 value=f(b["pick_value"][tp, j]), reward=r, mask=f(m),
                                 v_next=f(vn)))
                seen["span"] += tp < starts[c]
                seen["mask0" if m == 0 else "mask1"] += 1
                seen["survived"] += bool(b["done"][tp:tc, j].any())
            seen["no_rows"] += not rows
            an = f(0)
            for row in reversed(rows):
                m = row["mask"]
                delta = row["reward"] + row["v_next"] * m - row["value"]
                row["adv"] = f(delta + lam * an * m)
                an = row["adv"]
            out[c][j] = rows
    return out, seen
