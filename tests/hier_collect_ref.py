"""TEST INFRASTRUCTURE -- the numpy restatement of zenv_collect_hier's bookkeeping (checker only), shared by
tests/test_gpu_hier_collect.py and tests/test_gpu_hier_shapes.py: `replay` drives a second handle frame by frame with
zenv_policy(HIER_SAMPLE) + zenv_step and records what a collection sees; `expected_hi` turns that record into the
high-level rows of every call (_hier_policy_opt.py:66-76, 98-107)."""
import numpy as np

LAM, GAMMA = 0.95, 0.99


def replay(Z, env, frames, seed):
    """Drive `env` with zenv_policy(HIER_SAMPLE) + zenv_step for `frames` frames; the per-frame record."""
    log = {k: [] for k in ("obs", "zone_obs", "need", "avail", "goal", "pick_value", "logits", "action", "mu", "std",
                           "value", "reward", "done", "shaped", "need_after")}
    for _ in range(frames):
        o, zo = env.observations()
        _, need, avail, _ = env.goal_info()
        env.policy(Z.POLICY_HIER_SAMPLE, policy_seed=seed)
        log["obs"].append(o)
        log["zone_obs"].append(zo)
        log["need"].append(need)
        log["avail"].append(avail)
        log["goal"].append(env.get(Z.F_GOAL))
        log["pick_value"].append(env.get(Z.F_HIER_VALUE))
        log["logits"].append(env.get(Z.F_HIER_LOGITS))
        log["action"].append(env.get(Z.F_ACTIONS))
        log["mu"].append(env.get(Z.F_POLICY_MU))
        log["std"].append(env.get(Z.F_POLICY_STD))
        log["value"].append(env.get(Z.F_POLICY_VALUE))
        env.step(None, auto_reset=True)
        _, _, r, d, _ = env.results()
        sh, need_after, _, _ = env.goal_info()
        log["reward"].append(r)
        log["done"].append(d)
        log["shaped"].append(sh)
        log["need_after"].append(need_after)
    return {k: np.stack(v) for k, v in log.items()}


def log_softmax_at(logits, g):
    fin = np.isfinite(logits)
    l64 = logits.astype(np.float64)
    m = l64[fin].max()
    return l64[g] - m - np.log(np.exp(l64[fin] - m).sum())


def expected_hi(b, T, n_calls, v_final, dtype=np.float32):
    """The numpy restatement: per call, per env, the closed transitions in order with their GAE (_hier_policy_opt.py:
    66-76, 98-107).  T: frames per call, or a list of them (calls of different lengths); v_final[c] = V_hi(obs_T) after
    call c.  dtype: the arithmetic's (float32: the device's; float64 for a float64 recording).  Also returns what the
    call-boundary cases looked like."""
    f = dtype
    n = b["obs"].shape[1]
    starts = np.concatenate([[0], np.cumsum([T] * n_calls if np.isscalar(T) else T)]).astype(int)
    out = [[[] for _ in range(n)] for _ in range(n_calls)]
    seen = {"span": 0, "mask0": 0, "mask1": 0, "bootstrap": 0}
    for j in range(n):
        hr = f(0)
        open_t = None
        events = []                                        # (close frame, pick frame, reward, mask)
        picks = []
        for t in range(starts[-1]):
            if b["need"][t, j] and b["goal"][t, j] >= 0:
                assert open_t is None
                open_t = t
                picks.append(t)
            hr = f(hr + b["reward"][t, j])
            if b["need_after"][t, j]:
                if open_t is not None:
                    events.append((t, open_t, hr, 0.0 if b["done"][t, j] else 1.0))
                    open_t = None
                hr = f(0)
        for c in range(n_calls):
            closed = [e for e in events if starts[c] <= e[0] < starts[c + 1]]
            rows = []
            for k, (tc, tp, r, m) in enumerate(closed):
                nxt = [p for p in picks if p > tp]
                if nxt and nxt[0] < starts[c + 1]:
                    vn = b["pick_value"][nxt[0], j]
                else:
                    vn = v_final[c][j]
                    seen["bootstrap"] += m == 1.0                # V_hi(obs_T) enters this row's advantage
                rows.append(dict(t_pick=tp, t_close=tc, goal=b["goal"][tp, j], value=b["pick_value"][tp, j], reward=r,
                                 mask=f(m), v_next=f(vn)))
                seen["span"] += tp < starts[c]
                seen["mask0" if m == 0 else "mask1"] += 1
            an = f(0)
            for row in reversed(rows):
                m = row["mask"]
                delta = row["reward"] + row["v_next"] * m - row["value"]
                row["adv"] = f(delta + f(LAM) * an * m)
                an = row["adv"]
            out[c][j] = rows
    return out, seen
