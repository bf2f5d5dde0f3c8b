"""Record what the reference's own agent code computes, as fixtures for tests/test_agent_goldens_cpu.py and
tests/test_gpu_agent_goldens.py.

The reference's environments need MuJoCo, which is not here; its agents are plain torch.  This script imports them at
run time -- the models, ``collect_experiences`` and the update functions of the four variants (main, zone-goals,
xy-goals, options) -- behind a few stand-in modules (a ``gym`` whose spaces carry low / high / shape / n, and empty
permissive modules for glfw, mujoco_py, safety_gym and gym.envs.registration), drives them on inputs it builds itself
and stores only the data they consume and produce.  Nothing of the reference's text is copied: the stand-ins, the toy
environments and the experience builders below are this project's own code.

Every variant runs in fresh child processes (the variants reuse module names), started with ``python -B`` so that no
bytecode cache is written into the reference tree.  Each item is recorded twice: in float32, the reference as it
stands, and in float64 (``torch.set_default_dtype(torch.float64)``, the same float32 weights and inputs widened) as the
high-precision yardstick.  torch, numpy.random and random are seeded; everything the reference drew (actions, goals,
skills, termination draws, minibatch index lists) is stored, so no test reproduces an RNG stream.

Run (needs the reference tree, by default /root/reference, else $ZENV_REFERENCE):

    python tests/golden/make_agent_goldens.py            writes tests/golden/agent_<variant>_<part>.npz

One run writes the whole set, and a set is self-consistent: the recorded inputs of the updates are derived from the
float32 models' own recorded outputs.  Another CPU or BLAS moves the float32 run by float32 ulps -- up to 3e-6 of an
array's maximum has been seen between two machines -- which is far beyond the 1e-9 float64 bound of the tests.  So sets
from different machines are never mixed: regenerate and commit all agent_*.npz files together.  Not collected by
pytest; the tests read only the .npz files.
"""
import os
import pickle
import random
import subprocess
import sys
import tempfile
import types

import numpy as np


def _agent_goldens():
    """tests/agent_goldens.py by its path: the children put the reference's directories first on sys.path."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "agent_goldens.py")
    spec = importlib.util.spec_from_file_location("zenv_tests_agent_goldens", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_AG = _agent_goldens()
sketch, SMALL = _AG.sketch, _AG.SMALL                # the probes are defined once, there; SMALL: see drive_update

REFERENCE = os.environ.get("ZENV_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = ("main", "zone-goals", "xy-goals", "options")
H = 32                                               # h_dim of every recorded model
TSP = (15, 6)                                        # PointTSP-v0: Z zones, F features per zone row
CM = (6, 7)                                          # ColourMatch-v0
N_SKILLS = 5
B_NET = 12                                           # rows of a network-forward batch
SEED = 20240607
LIMIT_FILE, LIMIT_ALL = 256 * 1024, 1024 * 1024


# ------------------------------------------------------------------------------------------------ the stand-in modules
def install_stand_ins():
    """A gym with the spaces the models look at, and permissive empty modules for what the env files import."""

    class Anything:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return Anything()

        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return Anything()

    class Permissive(types.ModuleType):
        __path__ = []

        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            cls = type(name, (Anything,), {})
            setattr(self, name, cls)
            return cls

    class Box:
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.shape = tuple(shape) if shape is not None else np.shape(low)
            self.low = np.full(self.shape, low, np.float32)
            self.high = np.full(self.shape, high, np.float32)

    class Discrete:
        def __init__(self, n):
            self.n, self.shape = int(n), ()

    class Dict:
        def __init__(self, spaces):
            self.spaces = dict(spaces)

    class Env:
        @property
        def unwrapped(self):
            return self

    class Wrapper(Env):
        def __init__(self, env):
            self.env = env
            self.observation_space, self.action_space = env.observation_space, env.action_space

        def __getattr__(self, name):
            if name.startswith("_") or name == "env":
                raise AttributeError(name)
            return getattr(self.env, name)

        @property
        def unwrapped(self):
            return self.env.unwrapped

        def step(self, action):
            return self.env.step(action)

        def reset(self):
            return self.env.reset()

    gym = Permissive("gym")
    gym.Env, gym.Wrapper = Env, Wrapper
    spaces = Permissive("gym.spaces")
    spaces.Box, spaces.Discrete, spaces.Dict = Box, Discrete, Dict
    gym.spaces = spaces
    mods = {"gym": gym, "gym.spaces": spaces}
    for name in ("gym.envs", "gym.envs.registration", "glfw", "mujoco_py", "safety_gym", "safety_gym.envs",
                 "safety_gym.envs.engine", "safety_gym.random_agent"):
        mods[name] = Permissive(name)
    sys.modules.update(mods)
    return spaces


def enter_variant(variant):
    root = os.path.join(REFERENCE, variant)
    sys.path[:0] = [os.path.join(root, "src"), root]
    return install_stand_ins()


def seed_all(offset=0):
    import torch
    torch.manual_seed(SEED + offset)
    np.random.seed(SEED + offset)
    random.seed(SEED + offset)


# ------------------------------------------------------------------------------------------------ shared helpers
def np_of(t):
    return t.detach().cpu().numpy().copy()


def state_dict_np(model):
    return {k: np_of(v) for k, v in model.state_dict().items()}


def randomise_biases(model, offset):
    """init_params leaves every bias 0; small random ones make the bias paths count."""
    import torch
    g = torch.Generator().manual_seed(SEED + 77 + offset)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float32))


def spaces_for(spaces, Z, F):
    obs_space = spaces.Dict({"obs": spaces.Box(-np.inf, np.inf, (8,)), "zone_obs": spaces.Box(-np.inf, np.inf, (Z, F))})
    return obs_space, spaces.Box(-1, 1, (2,))


def random_obs(n, Z, F, offset):
    """float32 obs [n, 8] and zone rows [n, Z, F]."""
    import torch
    g = torch.Generator().manual_seed(SEED + 500 + offset)
    f32 = torch.float32
    return torch.randn((n, 8), generator=g, dtype=f32), torch.rand((n, Z, F), generator=g, dtype=f32) * 2.0 - 1.0


def widen(x, dtype):
    import torch
    if isinstance(x, torch.Tensor):
        return x.to(dtype) if x.is_floating_point() else x
    if isinstance(x, dict):
        return type(x)({k: widen(v, dtype) for k, v in x.items()})
    return x


class Recorder:
    """What one child returns: name -> array, under '<item>/<f32|f64>/<name>' or '<item>/<name>' for what both share."""

    def __init__(self, prec):
        self.prec, self.out = prec, {}

    def both(self, item, name, a):
        self.out[f"{item}/{name}"] = np.asarray(a)

    def mine(self, item, name, a):
        self.out[f"{item}/{self.prec}/{name}"] = np.asarray(a)


def hooked_raw(module):
    """The raw output of `module` (the actor's last Linear) at its next forward: Categorical(logits=...) keeps only the
    normalised logits, the restatements return the raw ones."""
    box = []
    handle = module.register_forward_hook(lambda m, i, o: box.append(o.detach().clone()))
    return box, handle


def drive_update(rec, item, update, optimizer, model, index_fn_owner, index_fn_name, full, minibatches=2):
    """Run `update` (a bound update_* method of the reference's algorithm object) for `minibatches` optimizer steps:
    the index lists it drew, the gradient of every parameter at the first step, the per-minibatch statistics, and the
    parameters and Adam moments after the last step.  The fixtures have to stay under 1 MiB together, and one model of
    h_dim 32 is 25 KiB in float32: the gradients of every parameter are kept only where `full` (the flat-plain and
    Zone-goals learners), elsewhere -- and for the state after the last step everywhere -- only the tensors of at most SMALL
    elements are: every bias and every head, which every term of the loss and every setting of the optimizer reach.  A
    larger gradient that is not kept in full is kept as its sketch [G v, u^T G] (tests/agent_goldens.sketch), computed
    in float64 from this precision's gradient."""
    drawn, grads, steps = [], {}, [0]
    names = [k for k, _ in model.named_parameters()]
    inner_index = getattr(index_fn_owner, index_fn_name)

    def index_fn(*a, **k):
        out = [np.asarray(b).copy() for b in inner_index(*a, **k)]
        drawn.extend(out)
        return out[:minibatches]

    inner_step = optimizer.step

    def step(*a, **k):
        if steps[0] == 0:
            for n, p in zip(names, model.parameters()):
                grads[n] = np_of(p.grad)
        steps[0] += 1
        return inner_step(*a, **k)

    setattr(index_fn_owner, index_fn_name, index_fn)
    optimizer.step = step
    try:
        logs = update()
    finally:
        setattr(index_fn_owner, index_fn_name, inner_index)
        optimizer.step = inner_step
    assert steps[0] == minibatches, (item, steps)
    for i in range(minibatches):
        rec.both(item, f"index{i}", drawn[i].astype(np.int64))
    for n in names:
        if full or grads[n].size <= SMALL:
            rec.mine(item, f"grad/{n}", grads[n])
        else:
            rec.mine(item, f"sketch/{n}", sketch(grads[n]))
    after = dict(model.named_parameters())
    for n, p in zip(names, model.parameters()):
        if grads[n].size > SMALL:
            continue
        st = optimizer.state[p]
        rec.mine(item, f"param/{n}", np_of(after[n]))
        rec.mine(item, f"exp_avg/{n}", np_of(st["exp_avg"]))
        rec.mine(item, f"exp_avg_sq/{n}", np_of(st["exp_avg_sq"]))
    return logs


def wrap_logs(lists):
    """The reference's update functions hand out means over minibatches; the per-minibatch values are what
    numpy.mean / np.mean is given -- capture the lists on their way in."""
    import numpy
    inner = numpy.mean

    def mean(a, *args, **kw):
        lists.append(list(a))
        return inner(a, *args, **kw)

    numpy.mean = mean
    return lambda: setattr(numpy, "mean", inner)


def gaussian_experience(model_call, n, act_dim, offset):
    """A low-level / flat experience around the model's own outputs so that every loss branch is reached at the first
    minibatch (unchanged parameters: ratio = exp(new - old log_prob)).  model_call() -> (Normal, value) in float32.
    Rows i % 6: 0 ratio above the range with a positive advantage (clipped), 1 above with a negative one, 2 below with a
    negative one (clipped), 3 below with a positive one, 4 the recorded value 1 below (the clipped value term wins),
    5 the recorded value 1 above with the return beyond it (the unclipped term wins)."""
    import torch
    g = torch.Generator().manual_seed(SEED + 900 + offset)
    f32 = torch.float32
    with torch.no_grad():
        dist, value = model_call()
        value = value[0] if isinstance(value, tuple) else value
        action = dist.mean + dist.stddev * torch.randn(dist.mean.shape, generator=g, dtype=f32)
        lp = dist.log_prob(action)
    k = torch.arange(n) % 6
    d_old = 0.02 * torch.randn(n, generator=g, dtype=f32)
    d_old[(k == 0) | (k == 1)] = -0.5
    d_old[(k == 2) | (k == 3)] = 0.5
    adv = torch.randn(n, generator=g, dtype=f32)
    adv[k == 0] = adv[k == 0].abs() + 0.1
    adv[k == 1] = -adv[k == 1].abs() - 0.1
    adv[k == 2] = -adv[k == 2].abs() - 0.1
    adv[k == 3] = adv[k == 3].abs() + 0.1
    old_v = value + 0.05 * torch.randn(n, generator=g, dtype=f32)
    old_v[k == 4] = value[k == 4] - 1.0
    old_v[k == 5] = value[k == 5] + 1.0
    ret = old_v + adv
    ret[k == 4] = value[k == 4] + 0.05
    ret[k == 5] = old_v[k == 5] + 0.4
    old_lp = lp + (d_old / act_dim).view(-1, 1) if lp.dim() == 2 else lp + d_old
    return dict(action=action, log_prob=old_lp, value=old_v, advantage=adv, returnn=ret)


def branch_counts(new_lp, value, e, clip_eps):
    """How many rows of an experience take which branch at the recorded parameters (float32 tensors)."""
    import torch
    old = e["log_prob"].sum(dim=1) if e["log_prob"].dim() == 2 else e["log_prob"]
    ratio = torch.exp(new_lp - old)
    dv = value - e["value"]
    vc = e["value"] + dv.clamp(-clip_eps, clip_eps)
    clipped_wins = (vc - e["returnn"]).pow(2) > (value - e["returnn"]).pow(2)
    counts = {"ratio_clipped_high": int(((ratio > 1 + clip_eps) & (e["advantage"] > 0)).sum()),
              "ratio_clipped_low": int(((ratio < 1 - clip_eps) & (e["advantage"] < 0)).sum()),
              "ratio_unclipped": int(((ratio >= 1 - clip_eps) & (ratio <= 1 + clip_eps)).sum()),
              "value_clipped_term_larger": int(((dv.abs() > clip_eps) & clipped_wins).sum()),
              "value_unclipped_term_larger": int((~clipped_wins).sum())}
    assert all(v > 0 for v in counts.values()), counts
    return counts


def store_counts(rec, item, counts):
    for k, v in counts.items():
        rec.both(item, f"count/{k}", np.int64(v))


# ------------------------------------------------------------------------------------------------ the toy environments
def toy_obs(j, t, Z, F):
    """Deterministic float32 observations of env j at its step counter t: no physics, only distinct numbers."""
    a = np.arange(8, dtype=np.float64)
    z = np.arange(Z * F, dtype=np.float64).reshape(Z, F)
    return {"obs": np.sin(0.37 * a + 0.91 * j + 0.53 * t).astype(np.float32),
            "zone_obs": np.cos(0.11 * z + 0.29 * j + 0.17 * t).astype(np.float32)}


def toy_reward(j, t):
    return float(np.float32(np.sin(0.7 * j + 0.31 * t) + (1.0 if t % 5 == 0 else 0.0)))


def toy_shaped(j, t):
    return float(np.float32(0.1 * np.cos(0.3 * j + 0.23 * t)))


class ToyEnv:
    """A scripted stand-in with the surface the flat collector's ParallelEnv calls: reset, step, the two spaces.
    done_at: the step counters (counted over the env's whole life) at which an episode ends."""

    def __init__(self, spaces, j, Z, F, done_at, shaped=True):
        self.j, self.Z, self.F, self.t = j, Z, F, 0
        self.done_at, self.shaped = set(done_at), shaped
        self.observation_space, self.action_space = spaces_for(spaces, Z, F)

    @property
    def unwrapped(self):
        return self

    def reset(self):
        self.t += 1000                                    # a fresh episode's observations differ from the last one's
        return toy_obs(self.j, self.t, self.Z, self.F)

    def step(self, action):
        self.t += 1
        tt = self.t % 1000
        info = {"shaped_reward": toy_shaped(self.j, self.t)} if self.shaped else {}
        done = tt in self.done_at
        if done:
            self.done_at.discard(tt)
        return toy_obs(self.j, self.t, self.Z, self.F), toy_reward(self.j, self.t), done, info


class ToyGoalEnv(ToyEnv):
    """ToyEnv plus the goal surface of the Zone-goals environments: goal_zone, set_goal, get_goal, get_available_goals,
    info['need_next_goal'].  reach_at: the step counters at which the goal is reached (the transition closes without
    the episode ending); an episode's end closes it too."""

    goal_dim = 2

    def __init__(self, spaces, j, Z, F, done_at, reach_at):
        super().__init__(spaces, j, Z, F, done_at)
        self.reach_at, self.goal_zone, self.life = set(reach_at), None, 0

    def reset(self):
        self.goal_zone = None
        return super().reset()

    def step(self, action):
        assert self.goal_zone is not None
        self.life += 1
        obs, reward, done, info = super().step(action)
        reached = self.life in self.reach_at
        info["need_next_goal"] = bool(reached or done)
        if info["need_next_goal"]:
            self.goal_zone = None
        return obs, reward, done, info

    def set_goal(self, goal):
        self.goal_zone = int(goal)

    def get_goal(self):
        return np.array([np.sin(1.3 * self.goal_zone + 0.2 * self.j), np.cos(0.7 * self.goal_zone + 0.1 * self.t)]) / 3.0

    def get_available_goals(self):
        assert self.goal_zone is None
        k = np.arange(self.Z)
        avail = ((k * 7 + self.j * 3 + self.life) % 4) != 0
        avail[(self.j + self.life) % self.Z] = True
        return avail


def log_calls(penv, names, log):
    """Wrap methods of the reference's ParallelEnv object so that what the collector consumed is kept, per call."""
    for name in names:
        inner = getattr(penv, name)

        def call(*a, _inner=inner, _name=name, **k):
            out = _inner(*a, **k)
            if _name in ("step", "step_no_reset"):
                out = tuple(list(x) for x in out)
            log.append((_name, a, out))
            return out

        setattr(penv, name, call)


def obs_arrays(obss):
    return (np.stack([o["obs"] for o in obss]).astype(np.float32),
            np.stack([o["zone_obs"] for o in obss]).astype(np.float32))


def store_exps(rec, item, prefix, exps, skip=()):
    """Every field of a DictList of experiences, obs.* one level down."""
    import torch
    for k, v in dict.items(exps):
        if k in skip:
            continue
        if isinstance(v, dict):
            for kk, vv in dict.items(v):
                if kk != "zone_obs":                       # the stream has them; obs.obs is enough to see the row order
                    rec.mine(item, f"{prefix}.{k}.{kk}", np_of(vv))
        elif isinstance(v, torch.Tensor):
            rec.mine(item, f"{prefix}.{k}", np_of(v))


# ------------------------------------------------------------------------------------------------ the flat agent (main)
def flat_networks(rec, spaces, dtype):
    import torch
    from flat_model import ACModel
    import torch_ac
    models = {}
    for tag, (Z, F), dist_value in (("plain", TSP, False), ("dist", CM, True)):
        item = f"flat_{tag}"
        seed_all(1 + dist_value)
        torch.set_default_dtype(torch.float32)
        obs_space, action_space = spaces_for(spaces, Z, F)
        model = ACModel({k: v.shape for k, v in obs_space.spaces.items()}, action_space, H, dist_value)
        randomise_biases(model, 1 + dist_value)
        for k, v in state_dict_np(model).items():
            rec.both(item, f"sd/{k}", v)
        obs, zone_obs = random_obs(B_NET, Z, F, 1 + dist_value)
        rec.both(item, "in/obs", np_of(obs))
        rec.both(item, "in/zone_obs", np_of(zone_obs))
        torch.set_default_dtype(dtype)
        model = model.to(dtype)
        with torch.no_grad():
            dist, value = model(torch_ac.DictList({"obs": obs.to(dtype), "zone_obs": zone_obs.to(dtype)}))
        rec.mine(item, "out/mu", np_of(dist.mean))
        rec.mine(item, "out/std", np_of(dist.stddev))
        if dist_value:
            rec.mine(item, "out/value", np_of(value[0]))
            rec.mine(item, "out/value_sigma", np_of(value[1]))
        else:
            rec.mine(item, "out/value", np_of(value))
        models[tag] = (model, Z, F, dist_value)
    return models


FLAT_HYPER = dict(discount=0.99, lr=3e-4, gae_lambda=0.95, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=0.5,
                  adam_eps=1e-8, clip_eps=0.2)
FLAT_NT = (6, 8)                                    # envs x frames of the flat update's experience and collection


def flat_algo(spaces, model, Z, F, dist_value, dtype, done_at, batch_size):
    """The reference's PPOAlgo over toy environments, its observation preprocessor widened for the float64 run."""
    import torch
    import torch_ac
    from utils.format import get_obss_preprocessor
    N, T = FLAT_NT
    envs = [ToyEnv(spaces, j, Z, F, done_at[j]) for j in range(N)]
    _, pre = get_obss_preprocessor(envs[0].observation_space)
    algo = torch_ac.algos.PPOAlgo(envs, model, torch.device("cpu"), T, FLAT_HYPER["discount"], FLAT_HYPER["lr"],
                                  FLAT_HYPER["gae_lambda"], dist_value, FLAT_HYPER["entropy_coef"],
                                  FLAT_HYPER["value_loss_coef"], FLAT_HYPER["max_grad_norm"], 1, FLAT_HYPER["adam_eps"],
                                  FLAT_HYPER["clip_eps"], 1, batch_size, lambda o, device=None: widen(pre(o, device), dtype))
    return algo


def flat_update(rec, spaces, models, dtype):
    import torch
    import torch_ac
    N, T = FLAT_NT
    for tag, (model, Z, F, dist_value) in models.items():
        item = f"flat_{tag}_update"
        n = N * T
        obs, zone_obs = random_obs(n, Z, F, 10 + dist_value)
        f32 = model.to(torch.float32) if dtype != torch.float32 else model
        torch.set_default_dtype(torch.float32)
        e = gaussian_experience(lambda: f32(torch_ac.DictList({"obs": obs, "zone_obs": zone_obs})), n, 2, 10 + dist_value)
        with torch.no_grad():
            d, v = f32(torch_ac.DictList({"obs": obs, "zone_obs": zone_obs}))
            v = v[0] if dist_value else v
            counts = branch_counts(d.log_prob(e["action"]).sum(dim=1), v, e, FLAT_HYPER["clip_eps"])
        store_counts(rec, item, counts)
        torch.set_default_dtype(dtype)
        model = model.to(dtype)
        rec.both(item, "exp/obs", np_of(obs))
        rec.both(item, "exp/zone_obs", np_of(zone_obs))
        for k, a in e.items():
            rec.both(item, f"exp/{k}", np_of(a))
        for k, a in FLAT_HYPER.items():
            rec.both(item, f"hyper/{k}", np.float64(a))
        rec.both(item, "shape/NT", np.array([N, T], np.int64))
        algo = flat_algo(spaces, model, Z, F, dist_value, dtype, [()] * N, batch_size=20)
        exps = torch_ac.DictList({k: a.to(dtype) for k, a in e.items()})
        exps.obs = torch_ac.DictList({"obs": obs.to(dtype), "zone_obs": zone_obs.to(dtype)})
        seed_all(20 + dist_value)
        lists = []
        undo = wrap_logs(lists)
        try:
            drive_update(rec, item, lambda: algo.update_parameters(exps), algo.optimizer, model, algo,
                         "_get_batches_starting_indexes", full=not dist_value)
        finally:
            undo()
        names = ["entropy", "value"] + (["value_std"] if dist_value else []) + ["policy_loss", "value_loss", "grad_norm"]
        assert len(lists) == len(names)
        for name, values in zip(names, lists):
            rec.mine(item, f"log/{name}", np.array(values, np.float64))


def flat_collect(rec, spaces, models, dtype):
    """Two consecutive collect_experiences calls of the reference's BaseAlgo over scripted toy environments."""
    import torch
    model, Z, F, dist_value = models["plain"]
    N, T = FLAT_NT
    item = "flat_collect"
    # env 0 never ends; 1 ends inside the first window; 2 on the first window's last frame; 3 on the second window's
    # first frame; 4 twice in one window; 5 on the very last frame
    done_at = [(), (3,), (T,), (T + 1,), (2, 5), (2 * T,)]
    algo = flat_algo(spaces, model.to(dtype), Z, F, dist_value, dtype, done_at, batch_size=16)
    log = [("reset", (), algo.obs)]
    log_calls(algo.env, ("step",), log)
    values = []
    handle = model.register_forward_hook(lambda m, i, o: values.append(np_of(o[1])))
    seed_all(30)
    for call in range(2):
        exps, _ = algo.collect_experiences()
        store_exps(rec, item, f"call{call}/exps", exps)
        rec.mine(item, f"call{call}/next_value", values[-1])
        rec.mine(item, f"call{call}/cur_mask", np_of(algo.mask))
        rec.mine(item, f"call{call}/masks", np_of(algo.masks))
    handle.remove()
    steps = [x for x in log if x[0] == "step"]
    assert len(steps) == 2 * T
    obs0, zone0 = obs_arrays(log[0][2])
    rec.both(item, "stream/obs", np.stack([obs0] + [obs_arrays(s[2][0])[0] for s in steps]))       # [2T + 1, N, 8]
    rec.both(item, "stream/zone_obs", np.stack([zone0] + [obs_arrays(s[2][0])[1] for s in steps]))
    rec.both(item, "stream/reward", np.array([s[2][1] for s in steps], np.float64))                  # [2T, N]
    rec.both(item, "stream/done", np.array([s[2][2] for s in steps], bool))
    rec.both(item, "stream/shaped_reward", np.array([[i["shaped_reward"] for i in s[2][3]] for s in steps], np.float64))
    rec.mine(item, "stream/action", np.stack([np.asarray(s[1][0]) for s in steps]))
    rec.both(item, "shape/NT", np.array([N, T], np.int64))
    rec.both(item, "hyper/discount", np.float64(FLAT_HYPER["discount"]))
    rec.both(item, "hyper/gae_lambda", np.float64(FLAT_HYPER["gae_lambda"]))
    d = np.array([s[2][2] for s in steps], bool)
    frame = np.arange(2 * T) % T
    counts = {"episode_end_inside_window": int(d[(frame > 0) & (frame < T - 1)].sum()),
              "episode_end_on_window_last_frame": int(d[frame == T - 1].sum()),
              "episode_end_on_window_first_frame": int(d[frame == 0].sum()),
              "env_without_episode_end": int((d.sum(axis=0) == 0).sum())}
    assert all(v > 0 for v in counts.values()), counts
    store_counts(rec, item, counts)
    assert d[:, 0].sum() == 0 and d[T - 1, 2] and d[T, 3] and d[:T, 4].sum() == 2 and d[2 * T - 1, 5]


# ------------------------------------------------------------------------------------------------ the hierarchical agents
def perturb(lp, value, offset):
    """gaussian_experience's rows for any policy: (old log_prob summed over the action, value, advantage, returnn)."""
    import torch
    g = torch.Generator().manual_seed(SEED + 950 + offset)
    f32, n = torch.float32, lp.shape[0]
    k = torch.arange(n) % 6
    d_old = 0.02 * torch.randn(n, generator=g, dtype=f32)
    d_old[(k == 0) | (k == 1)] = -0.5
    d_old[(k == 2) | (k == 3)] = 0.5
    adv = torch.randn(n, generator=g, dtype=f32)
    for kk, sign in ((0, 1.0), (1, -1.0), (2, -1.0), (3, 1.0)):
        adv[k == kk] = sign * (adv[k == kk].abs() + 0.1)
    old_v = value + 0.05 * torch.randn(n, generator=g, dtype=f32)
    old_v[k == 4] = value[k == 4] - 1.0
    old_v[k == 5] = value[k == 5] + 1.0
    ret = old_v + adv
    ret[k == 4] = value[k == 4] + 0.05
    ret[k == 5] = old_v[k == 5] + 0.4
    return lp + d_old, old_v, adv, ret


def two_level_networks(rec, agent, hi, lo, Z, F, lo_extra, dtype, hi_raw=None):
    """state_dicts, inputs and outputs of a (high, low) pair.  lo_extra: name -> float32 / int64 tensor [B_NET] that the
    low level's observation carries besides obs and zone_obs (goal or skill).  hi_raw: the module whose output is the
    high level's raw logits, where its policy is categorical."""
    import torch
    import torch_ac
    for level, model in (("hi", hi), ("lo", lo)):
        randomise_biases(model, 40 + len(agent) + (level == "lo"))
        for k, v in state_dict_np(model).items():
            rec.both(agent, f"{level}_sd/{k}", v)
    obs, zone_obs = random_obs(B_NET, Z, F, 40 + len(agent))
    rec.both(agent, "in/obs", np_of(obs))
    rec.both(agent, "in/zone_obs", np_of(zone_obs))
    for k, v in lo_extra.items():
        rec.both(agent, f"in/{k}", np_of(v))
    torch.set_default_dtype(dtype)
    hi.to(dtype), lo.to(dtype)
    x = torch_ac.DictList({"obs": obs.to(dtype), "zone_obs": zone_obs.to(dtype)})
    with torch.no_grad():
        if hi_raw is not None:
            box, handle = hooked_raw(hi_raw)
        dist, value = hi(x)
        if hi_raw is not None:
            handle.remove()
            rec.mine(agent, "hi_out/raw_logits", np_of(box[0]).reshape(B_NET, -1))
            rec.mine(agent, "hi_out/logits", np_of(dist.logits))
        else:
            rec.mine(agent, "hi_out/mu", np_of(dist.mean))
            rec.mine(agent, "hi_out/std", np_of(dist.stddev))
        rec.mine(agent, "hi_out/value", np_of(value))
        for k, v in lo_extra.items():
            dict.__setitem__(x, k, widen(v, dtype))
        dist, value = lo(x)
        rec.mine(agent, "lo_out/mu", np_of(dist.mean))
        rec.mine(agent, "lo_out/std", np_of(dist.stddev))
        rec.mine(agent, "lo_out/value", np_of(value))
    return obs, zone_obs, dist


ZG_HYPER = dict(lr=3e-4, gae_lambda=0.95, entropy_coef=0.003, discount=0.99, value_loss_coef=0.5, clip_eps=0.2,
                hi_entropy_coef=0.01, hi_value_coef=0.5, hi_lr=3e-4, max_grad_norm=0.5, optim_eps=1e-8)
ZG_NT, ZG_M = (6, 9), 30                            # lo rows: N (T - 1) = 48; hi rows: M


def child_zone_goals(rec, spaces, dtype):
    import torch
    import torch_ac
    from hier_policy_value_models import HighPolicyValueModel, LoPolicyValueModel
    from utils.format import get_obss_preprocessor
    agent, (Z, F), f32 = "zone_goals", TSP, torch.float32
    seed_all(3)
    obs_space, action_space = spaces_for(spaces, Z, F)
    shapes, pre = get_obss_preprocessor(obs_space)
    hi = HighPolicyValueModel(dict(shapes), Z, H)
    lo = LoPolicyValueModel(dict(shapes), action_space, 2, H)
    g = torch.Generator().manual_seed(SEED + 41)
    goal = torch.rand((B_NET, 2), generator=g, dtype=f32) * 2.0 - 1.0
    obs, zone_obs, _ = two_level_networks(rec, agent, hi, lo, Z, F, {"goal": goal}, dtype, hi_raw=hi.actor)
    # masked goals, as the collector and the update mask them: -inf into the normalised logits, a second Categorical
    avail = torch.rand((B_NET, Z), generator=g, dtype=f32) < 0.5
    avail[torch.arange(B_NET), torch.arange(B_NET) % Z] = True
    avail[0] = False
    avail[0, 3] = True                                    # a single available goal
    avail[1] = True                                       # all of them
    with torch.no_grad():
        dist, _ = hi(torch_ac.DictList({"obs": obs.to(dtype), "zone_obs": zone_obs.to(dtype)}))
        dist.logits[~avail] = float("-inf")
        masked = torch.distributions.Categorical(logits=dist.logits)
    rec.both(agent, "in/available", avail.numpy())
    rec.mine(agent, "hi_out/masked_logits", np_of(masked.logits))
    store_counts(rec, agent, {"masked_goals": int((~avail).sum()), "rows_with_one_goal": int((avail.sum(1) == 1).sum()),
                              "rows_with_every_goal": int(avail.all(1).sum())})

    # ---- one update of each level on an experience built around the float32 models' own outputs
    N, T = ZG_NT
    n, M = N * (T - 1), ZG_M
    torch.set_default_dtype(f32)
    hi.to(f32), lo.to(f32)
    lo_obs, lo_zone = random_obs(n, Z, F, 42)
    lo_goal = torch.rand((n, 2), generator=g, dtype=f32) * 2.0 - 1.0
    hi_obs, hi_zone = random_obs(M, Z, F, 43)
    mask = torch.rand((M, Z), generator=g, dtype=f32) < 0.6
    mask[torch.arange(M), torch.arange(M) % Z] = True
    mask[0] = False
    mask[0, 5] = True
    mask[1] = True
    with torch.no_grad():
        lo_x = torch_ac.DictList({"obs": lo_obs, "zone_obs": lo_zone, "goal": lo_goal})
        d, v = lo(lo_x)
        action = d.mean + d.stddev * torch.randn(d.mean.shape, generator=g, dtype=f32)
        lp = d.log_prob(action)
        old, old_v, adv, ret = perturb(lp.sum(1), v, 1)
        lo_e = dict(action=action, log_prob=lp + ((old - lp.sum(1)) / 2).view(-1, 1), value=old_v, advantage=adv,
                    returnn=ret)
        store_counts(rec, "zone_goals_lo_update", branch_counts(lp.sum(1), v, lo_e, ZG_HYPER["clip_eps"]))
        hd, hv = hi(torch_ac.DictList({"obs": hi_obs, "zone_obs": hi_zone}))
        hd.logits[~mask] = float("-inf")
        hd = torch.distributions.Categorical(logits=hd.logits)
        u = torch.rand(M, generator=g, dtype=f32)
        ha = (hd.probs.cumsum(1) < u.view(-1, 1)).sum(1).clamp(max=Z - 1)
        ha = torch.where(mask.gather(1, ha.view(-1, 1)).squeeze(1), ha, mask.long().argmax(1))
        hlp = hd.log_prob(ha)
        old, old_v, adv, ret = perturb(hlp, hv, 2)
        hi_e = dict(action=ha, action_mask=mask, log_prob=old, value=old_v, advantage=adv, returnn=ret)
        counts = branch_counts(hlp, hv, hi_e, ZG_HYPER["clip_eps"])
        counts["masked_goals"] = int((~mask).sum())
        store_counts(rec, "zone_goals_hi_update", counts)
    for item, e, xs in (("zone_goals_lo_update", lo_e, dict(obs=lo_obs, zone_obs=lo_zone, goal=lo_goal)),
                        ("zone_goals_hi_update", hi_e, dict(obs=hi_obs, zone_obs=hi_zone))):
        for k, a in {**xs, **e}.items():
            rec.both(item, f"exp/{k}", np_of(a))
        for k, a in ZG_HYPER.items():
            rec.both(item, f"hyper/{k}", np.float64(a))
        rec.both(item, "shape/NT", np.array([N, T], np.int64))
    torch.set_default_dtype(dtype)
    hi.to(dtype), lo.to(dtype)
    algo = torch_ac.algos.HierPolicyAlgo([ToyGoalEnv(spaces, 0, Z, F, (), ())], hi, lo, torch.device("cpu"),
                                         lambda o, device=None: widen(pre(o, device), dtype), 1, 20, T,
                                         ZG_HYPER["lr"], ZG_HYPER["gae_lambda"], ZG_HYPER["entropy_coef"],
                                         ZG_HYPER["discount"], ZG_HYPER["value_loss_coef"], ZG_HYPER["clip_eps"], 1, 12,
                                         ZG_HYPER["hi_entropy_coef"], ZG_HYPER["hi_value_coef"], ZG_HYPER["hi_lr"],
                                         ZG_HYPER["max_grad_norm"], ZG_HYPER["optim_eps"])
    algo.num_frames_lo, algo.num_frames_hi = n, M         # what a collection of N envs x T frames with M rows leaves
    lo_exps = torch_ac.DictList({k: a.to(dtype) for k, a in lo_e.items()})
    lo_exps.obs = widen(lo_x, dtype)
    hi_exps = torch_ac.DictList({k: widen(a, dtype) for k, a in hi_e.items()})
    hi_exps.obs = torch_ac.DictList({"obs": hi_obs.to(dtype), "zone_obs": hi_zone.to(dtype)})
    for item, update, opt, model, fn in (
            ("zone_goals_hi_update", algo.update_hi_parameters, algo.hi_optimizer, hi, "_get_batches_starting_indexes_hi"),
            ("zone_goals_lo_update", algo.update_lo_parameters, algo.lo_optimizer, lo, "_get_batches_starting_indexes_lo")):
        seed_all(50 + len(item))
        lists = []
        undo = wrap_logs(lists)
        try:
            drive_update(rec, item, lambda: update((lo_exps, hi_exps)), opt, model, algo, fn, full=True)
        finally:
            undo()
        names = ("entropy", "value", "policy_loss", "value_loss", "grad_norm")
        assert len(lists) == len(names), (item, len(lists))
        for name, values in zip(names, lists):
            rec.mine(item, f"log/{name}", np.array(values, np.float64))
    seed_all(9)
    zone_goals_collect(rec, spaces, hi, lo, pre, dtype)


ZG_COLLECT_NT = (6, 8)


def zone_goals_collect(rec, spaces, hi, lo, pre, dtype):
    """Two consecutive collect_experiences calls of the Zone-goals HierPolicyAlgo over scripted ToyGoalEnvs, through
    the reference's own ParallelEnv: what it asked of the environments and got back, per frame, and what it made of it."""
    import torch
    import torch_ac
    item, (Z, F), (N, T) = "zone_goals_collect", TSP, ZG_COLLECT_NT
    # env 0 never closes a transition; 1: goal reached, then the episode ends inside the window; 2: the episode ends on
    # the first window's last frame; 3: goal reached on the very step the episode ends; 4: its first transition closes
    # in the second call, its second on that call's last frame (V_hi of the observation after the window enters); 5:
    # several transitions in a window, one closing on the first call's last frame, the episode ends on the very last frame
    done_at = [(), (3,), (T,), (5, 11), (), (2 * T,)]
    reach_at = [(), (2,), (4, 10), (5,), (T + 2, 2 * T), (3, T, 12)]
    h = ZG_HYPER
    envs = [ToyGoalEnv(spaces, j, Z, F, done_at[j], reach_at[j]) for j in range(N)]
    algo = torch_ac.algos.HierPolicyAlgo(envs, hi, lo, torch.device("cpu"), lambda o, device=None: widen(pre(o, device), dtype),
                                         1, 20, T, h["lr"], h["gae_lambda"], h["entropy_coef"], h["discount"],
                                         h["value_loss_coef"], h["clip_eps"], 1, 12, h["hi_entropy_coef"],
                                         h["hi_value_coef"], h["hi_lr"], h["max_grad_norm"], h["optim_eps"])
    log = [("reset", (), algo.obs)]
    log_calls(algo.env, ("needs_goal", "available_goals", "set_goal", "get_goal", "step"), log)
    hi_calls = []
    handle = hi.register_forward_hook(lambda m, i, o: hi_calls.append(np_of(o[1])))
    seed_all(33)
    frames = 2 * T
    need = np.zeros((frames, N), bool)
    goal = np.full((frames, N), -1, np.int64)
    avail = np.zeros((frames, N, Z), bool)
    goal_xy = np.zeros((frames, N, 2), np.float64)
    pick_value = np.zeros((frames, N), np.float64)
    v_final = []
    for call in range(2):
        n_log, n_hi = len(log), len(hi_calls)
        (lo_exps, hi_exps), _ = algo.collect_experiences()
        store_exps(rec, item, f"call{call}/lo_exps", lo_exps)
        store_exps(rec, item, f"call{call}/hi_exps", hi_exps)
        for name in ("lo_values", "lo_masks", "lo_rewards", "rewards", "lo_advantages"):
            rec.mine(item, f"call{call}/{name}", np_of(getattr(algo, name)))
        # the frames of this call: needs_goal opens one; the high level ran on the needing envs (if any), then on all
        t, k = call * T - 1, n_hi
        for name, a, out in log[n_log:]:
            if name == "needs_goal":
                t += 1
                need[t] = out
                if any(out):
                    pick_value[t, np.nonzero(out)[0]] = hi_calls[k]
                    k += 1
                k += 1                                     # the end-of-frame call on every env
            elif name == "available_goals":
                avail[t, a[0]] = out
            elif name == "set_goal":
                goal[t, a[0]] = int(a[1])
            elif name == "get_goal":
                goal_xy[t, a[0]] = out
        assert t == (call + 1) * T - 1 and k == len(hi_calls)
        v_final.append(hi_calls[-1])
    handle.remove()
    steps = [x for x in log if x[0] == "step"]
    obs0, zone0 = obs_arrays(log[0][2])
    done = np.array([s[2][2] for s in steps], bool)
    need_after = np.array([[i["need_next_goal"] for i in s[2][3]] for s in steps], bool)
    rec.both(item, "stream/obs", np.stack([obs0] + [obs_arrays(s[2][0])[0] for s in steps]))
    rec.both(item, "stream/reward", np.array([s[2][1] for s in steps], np.float64))
    rec.both(item, "stream/shaped_reward", np.array([[i["shaped_reward"] for i in s[2][3]] for s in steps], np.float64))
    rec.both(item, "stream/done", done)
    rec.both(item, "stream/need_after", need_after)
    rec.both(item, "stream/need", need)
    rec.both(item, "stream/available", avail)
    rec.mine(item, "stream/goal", goal)
    rec.mine(item, "stream/goal_xy", goal_xy)
    rec.mine(item, "stream/pick_value", pick_value)
    rec.mine(item, "stream/v_final", np.stack(v_final))
    rec.both(item, "shape/NT", np.array([N, T], np.int64))
    rec.both(item, "hyper/discount", np.float64(h["discount"]))
    rec.both(item, "hyper/gae_lambda", np.float64(h["gae_lambda"]))
    # the scripted cases, counted from the stream that was consumed
    spans = 0
    for j in range(N):
        open_t = None
        for t in range(frames):
            if need[t, j]:
                open_t = t
            if need_after[t, j]:
                spans += open_t < T <= t
                open_t = None
    counts = {"transition_closed_by_episode_end": int((need_after & done).sum()),
              "transition_closed_by_reaching_the_goal": int((need_after & ~done).sum()),
              "transition_spanning_two_calls": int(spans),
              "env_that_never_closes_a_transition": int((need_after.sum(axis=0) == 0).sum()),
              "episode_end_inside_window": int(done[(np.arange(frames) % T) < T - 1].sum()),
              "episode_end_on_window_last_frame": int(done[(np.arange(frames) % T) == T - 1].sum()),
              "goal_reached_on_the_step_the_episode_ends": sum(len(set(a) & set(b)) for a, b in zip(done_at, reach_at)),
              "goal_reached_on_window_last_frame": int((need_after & ~done)[(np.arange(frames) % T) == T - 1].sum()),
              "masked_goals_at_a_pick": int((~avail[need]).sum())}
    assert all(v > 0 for v in counts.values()), counts
    store_counts(rec, item, counts)


SK_COLLECT = (5, 8, 4)                              # envs, frames per call, skill_len


def skills_collect(rec, spaces, algo_for, hi, lo, dtype):
    """Two consecutive collect_experiences calls of main's HierPolicyAlgo over the reference's WaitWrapper around
    scripted toy environments, through its own ParallelEnv (step on a window's last frame, step_no_reset elsewhere)."""
    import torch
    from envs.wrappers import WaitWrapper
    item, (Z, F), (N, T, L) = "skills_collect", TSP, SK_COLLECT
    # env 0 never ends; 1 ends in the middle of a skill (no-op frames follow); 2 on a skill's last frame; 3 in the middle
    # of the first call's second skill and again in the second call; 4 on the second call's first frame
    done_at = [(), (2,), (4,), (6, 11), (9,)]
    envs = [WaitWrapper(ToyEnv(spaces, j, Z, F, done_at[j])) for j in range(N)]
    algo = algo_for(envs, T, L)
    log = [("reset", (), algo.obs)]
    log_calls(algo.env, ("step", "step_no_reset"), log)
    hi_calls, lo_calls = [], []
    handles = [hi.register_forward_hook(lambda m, i, o: hi_calls.append(np_of(o[1]))),
               lo.register_forward_hook(lambda m, i, o: lo_calls.append(np_of(o[1])))]
    seed_all(34)
    for call in range(2):
        n_hi, n_lo = len(hi_calls), len(lo_calls)
        (lo_exps, hi_exps, inv_exps), logs = algo.collect_experiences()
        store_exps(rec, item, f"call{call}/lo_exps", lo_exps)
        store_exps(rec, item, f"call{call}/hi_exps", hi_exps)
        store_exps(rec, item, f"call{call}/inverse_exps", inv_exps)
        for name in ("lo_values", "lo_masks", "lo_rewards", "rewards", "lo_skills", "hi_values", "hi_rewards", "lo_mask"):
            rec.mine(item, f"call{call}/{name}", np_of(getattr(algo, name)))
        assert len(hi_calls) - n_hi == T // L + 1 and len(lo_calls) - n_lo == T + 1
        rec.mine(item, f"call{call}/next_hi_value", hi_calls[-1])
        rec.mine(item, f"call{call}/next_lo_value", lo_calls[-1])
        rec.both(item, f"call{call}/num_frames", np.int64(logs["num_frames"]))
    for h in handles:
        h.remove()
    steps = [x for x in log if x[0] != "reset"]
    assert [x[0] for x in steps] == (["step_no_reset"] * (L - 1) + ["step"]) * (2 * T // L)
    obs0, zone0 = obs_arrays(log[0][2])
    done = np.array([s[2][2] for s in steps], bool)
    rec.both(item, "stream/obs", np.stack([obs0] + [obs_arrays(s[2][0])[0] for s in steps]))
    rec.both(item, "stream/zone_obs", np.stack([zone0] + [obs_arrays(s[2][0])[1] for s in steps]))
    rec.both(item, "stream/reward", np.array([s[2][1] for s in steps], np.float64))
    rec.both(item, "stream/done", done)
    rec.both(item, "shape/NTL", np.array([N, T, L], np.int64))
    rec.both(item, "hyper/discount", np.float64(algo.discount))
    rec.both(item, "hyper/gae_lambda", np.float64(algo.gae_lambda))
    rec.both(item, "hyper/diversity_coef", np.float64(algo.diversity_coef))
    rec.mine(item, "skill_logits", np_of(algo.skill_logits))
    frame = np.arange(2 * T) % L
    first = done & ~np.concatenate([np.zeros((1, N), bool), done[:-1] & (frame[:-1] != L - 1)[:, None]])
    counts = {"episode_end_inside_a_skill": int(first[frame < L - 1].sum()),
              "episode_end_on_a_skill_last_frame": int(first[frame == L - 1].sum()),
              "noop_frames_after_an_episode_end": int((done & ~first).sum()),
              "env_without_episode_end": int((done.sum(axis=0) == 0).sum()),
              "episode_end_in_the_windows_last_skill": int(first[(np.arange(2 * T) % T) >= T - L].sum())}
    assert all(v > 0 for v in counts.values()), counts
    store_counts(rec, item, counts)


OP_COLLECT_NT = (6, 10)


def options_collect(rec, spaces, algo_for, hi, dtype):
    """Two consecutive collect_experiences calls of the Options HierPolicyAlgo over the reference's WaitWrapper around
    scripted toy environments.  What it drew is kept: the skills, the three-component actions, and every uniform of the
    termination test torch.rand(()) < sigmoid(4 a_2 - 3)."""
    import torch
    from envs.wrappers import WaitWrapper
    item, (Z, F), (N, T) = "options_collect", CM, OP_COLLECT_NT
    done_at = [(), (3, 6, 9, 12, 15, 18), (2, 4, 7, 11, 13, 17), (T,), (5, 2 * T), (1, 8, 14, 16)]
    envs = [WaitWrapper(ToyEnv(spaces, j, Z, F, done_at[j])) for j in range(N)]
    algo = algo_for(envs, T)
    frames = 2 * T
    pick = np.zeros((frames, N), bool)
    ended = np.zeros((frames, N), bool)
    skill = np.full((frames, N), -1, np.int64)
    stepped = [0]

    class Logged(list):
        def __setitem__(self, j, v):
            if v is None:
                ended[stepped[0] - 1, j] = True
            else:
                pick[stepped[0], j] = True
            list.__setitem__(self, j, v)

    algo.cur_skills = Logged(algo.cur_skills)
    log = [("reset", (), algo.obs)]
    inner_step = algo.env.step

    def step(actions):
        skill[stepped[0]] = [int(k) for k in algo.cur_skills]
        out = tuple(list(x) for x in inner_step(actions))
        log.append(("step", (actions,), out))
        stepped[0] += 1
        return out

    algo.env.step = step
    draws = []
    inner_rand = torch.rand

    def rand(*a, **k):
        out = inner_rand(*a, **k)
        if a == ((),):
            draws.append(float(out))
        return out

    hi_calls = []
    handle = hi.register_forward_hook(lambda m, i, o: hi_calls.append(np_of(o[1])))
    seed_all(35)
    torch.rand = rand
    pick_value = np.zeros((frames, N), np.float64)
    v_final = []
    try:
        for call in range(2):
            n_hi = len(hi_calls)
            (lo_exps, hi_exps), _ = algo.collect_experiences()
            store_exps(rec, item, f"call{call}/lo_exps", lo_exps)
            store_exps(rec, item, f"call{call}/hi_exps", hi_exps)
            for name in ("lo_values", "lo_masks", "lo_rewards", "lo_actions", "lo_advantages"):
                rec.mine(item, f"call{call}/{name}", np_of(getattr(algo, name)))
            k = n_hi
            for t in range(call * T, (call + 1) * T):
                if pick[t].any():
                    pick_value[t, np.nonzero(pick[t])[0]] = hi_calls[k]
                    k += 1
            assert k == len(hi_calls) - 1
            v_final.append(hi_calls[-1])
    finally:
        torch.rand = inner_rand
        handle.remove()
    steps = [x for x in log if x[0] == "step"]
    assert len(steps) == frames and len(draws) == frames * N
    done = np.array([s[2][2] for s in steps], bool)
    obs0, _ = obs_arrays(log[0][2])
    rec.both(item, "stream/obs", np.stack([obs0] + [obs_arrays(s[2][0])[0] for s in steps]))
    rec.both(item, "stream/reward", np.array([s[2][1] for s in steps], np.float64))
    rec.both(item, "stream/done", done)
    rec.mine(item, "stream/pick", pick)
    rec.mine(item, "stream/ended", ended)
    rec.mine(item, "stream/skill", skill)
    rec.mine(item, "stream/term_uniform", np.array(draws, np.float64).reshape(frames, N))
    rec.mine(item, "stream/pick_value", pick_value)
    rec.mine(item, "stream/v_final", np.stack(v_final))
    rec.both(item, "shape/NT", np.array([N, T], np.int64))
    rec.both(item, "hyper/discount", np.float64(algo.discount))
    rec.both(item, "hyper/gae_lambda", np.float64(algo.gae_lambda))
    counts = {"option_ended_by_its_own_termination": int((ended & ~done).sum()),
              "option_ended_on_an_episode_end": int((ended & done).sum()),
              "option_surviving_an_episode_end": int((done & ~ended).sum()),
              "env_frames_without_a_pick": int((~pick).sum())}
    assert all(v > 0 for v in counts.values()), counts
    for k, v in counts.items():
        rec.mine(item, f"count/{k}", np.int64(v))          # the two precisions draw differently: a count each


XY_COLLECT = (5, 8, 4)                              # envs, frames per call, skill_len


def xy_collect(rec, spaces, algo_for, hi, lo, dtype):
    """Two consecutive collect_experiences calls of the xy-goals HierPolicyAlgo over the reference's WaitWrapper around
    scripted toy environments (step on a window's last frame, step_no_reset elsewhere)."""
    from envs.wrappers import WaitWrapper
    item, (Z, F), (N, T, L) = "xy_goals_collect", CM, XY_COLLECT
    # env 0 never ends; 1 ends in the middle of a goal's window (no-op frames follow); 2 on a window's last frame; 3 in
    # the middle of the first call's second window and again in the second call; 4 on the second call's first frame
    done_at = [(), (2,), (4,), (6, 11), (9,)]
    envs = [WaitWrapper(ToyEnv(spaces, j, Z, F, done_at[j])) for j in range(N)]
    algo = algo_for(envs, T, L)
    log = [("reset", (), algo.obs)]
    log_calls(algo.env, ("step", "step_no_reset"), log)
    hi_calls, lo_calls = [], []
    handles = [hi.register_forward_hook(lambda m, i, o: hi_calls.append(np_of(o[1]))),
               lo.register_forward_hook(lambda m, i, o: lo_calls.append(np_of(o[1])))]
    seed_all(36)
    for call in range(2):
        n_hi, n_lo = len(hi_calls), len(lo_calls)
        (lo_exps, hi_exps), logs = algo.collect_experiences()
        store_exps(rec, item, f"call{call}/lo_exps", lo_exps)
        store_exps(rec, item, f"call{call}/hi_exps", hi_exps)
        for name in ("lo_values", "lo_masks", "rewards", "lo_goals", "lo_dists_to_goal", "hi_goals", "hi_values",
                     "hi_rewards", "hi_log_probs", "lo_mask"):
            rec.mine(item, f"call{call}/{name}", np_of(getattr(algo, name)))
        assert len(hi_calls) - n_hi == T // L + 1 and len(lo_calls) - n_lo == T + 1
        rec.mine(item, f"call{call}/next_hi_value", hi_calls[-1])
        rec.mine(item, f"call{call}/next_lo_value", lo_calls[-1])
        rec.both(item, f"call{call}/num_frames", np.int64(logs["num_frames"]))
    for h in handles:
        h.remove()
    steps = [x for x in log if x[0] != "reset"]
    assert [x[0] for x in steps] == (["step_no_reset"] * (L - 1) + ["step"]) * (2 * T // L)
    obs0, zone0 = obs_arrays(log[0][2])
    done = np.array([s[2][2] for s in steps], bool)
    rec.both(item, "stream/obs", np.stack([obs0] + [obs_arrays(s[2][0])[0] for s in steps]))
    rec.both(item, "stream/zone_obs", np.stack([zone0] + [obs_arrays(s[2][0])[1] for s in steps]))
    rec.both(item, "stream/reward", np.array([s[2][1] for s in steps], np.float64))
    rec.both(item, "stream/done", done)
    rec.both(item, "shape/NTL", np.array([N, T, L], np.int64))
    rec.both(item, "hyper/discount", np.float64(algo.discount))
    rec.both(item, "hyper/gae_lambda", np.float64(algo.gae_lambda))
    frame = np.arange(2 * T) % L
    first = done & ~np.concatenate([np.zeros((1, N), bool), done[:-1] & (frame[:-1] != L - 1)[:, None]])
    counts = {"episode_end_inside_a_window": int(first[frame < L - 1].sum()),
              "episode_end_on_a_window_last_frame": int(first[frame == L - 1].sum()),
              "noop_frames_after_an_episode_end": int((done & ~first).sum()),
              "env_without_episode_end": int((done.sum(axis=0) == 0).sum()),
              "episode_end_in_the_calls_last_window": int(first[(np.arange(2 * T) % T) >= T - L].sum())}
    assert all(v > 0 for v in counts.values()), counts
    store_counts(rec, item, counts)


UPD_NT, UPD_M = (6, 8), 24                          # the other agents' update experiences: N x T low rows, M high rows
ABSENT_SKILL = 3                                    # a skill / option with no sample in either batch


def two_level_updates(rec, spaces, agent, hi, lo, Z, F, dtype, kind, make_algo):
    """One update of each level of the xy-goals (kind "goal"), fixed-length-skills ("skill") or Options ("option")
    agent by the reference's own update_hi_parameters / update_lo_parameters, on experiences built around the float32
    models' own outputs (perturb's rows).  -> (algo, hi_e): the algorithm object and the high-level experience."""
    import torch
    import torch_ac
    f32 = torch.float32
    N, T = UPD_NT
    n, M = N * T, UPD_M
    g = torch.Generator().manual_seed(SEED + 300 + len(agent))
    torch.set_default_dtype(f32)
    hi.to(f32), lo.to(f32)
    lo_obs, lo_zone = random_obs(n, Z, F, 70 + len(agent))
    hi_obs, hi_zone = random_obs(M, Z, F, 71 + len(agent))
    present = torch.tensor([k for k in range(N_SKILLS) if k != ABSENT_SKILL])
    if kind == "goal":
        extra = {"goal": torch.rand((n, 2), generator=g, dtype=f32) * 2.0 - 1.0}
    else:
        extra = {"skill": present[torch.arange(n) % len(present)]}
    with torch.no_grad():
        lo_x = torch_ac.DictList({"obs": lo_obs, "zone_obs": lo_zone, **extra})
        d, v = lo(lo_x)
        action = d.mean + d.stddev * torch.randn(d.mean.shape, generator=g, dtype=f32)
        lp = d.log_prob(action)
        old, old_v, adv, ret = perturb(lp.sum(1), v, 10 + len(agent))
        lo_e = dict(action=action, log_prob=lp + ((old - lp.sum(1)) / lp.shape[1]).view(-1, 1), value=old_v,
                    advantage=adv, returnn=ret)
        counts = branch_counts(lp.sum(1), v, lo_e, ZG_HYPER["clip_eps"])
        if kind != "goal":
            counts["skills_without_a_sample"] = N_SKILLS - len(set(extra["skill"].tolist()))
            assert counts["skills_without_a_sample"] > 0
        store_counts(rec, f"{agent}_lo_update", counts)
        hd, hv = hi(torch_ac.DictList({"obs": hi_obs, "zone_obs": hi_zone}))
        if kind == "goal":
            goal = hd.mean + hd.stddev * torch.randn(hd.mean.shape, generator=g, dtype=f32)
            hlp = hd.log_prob(goal).sum(-1)
            hi_e = dict(goal=goal)
        else:
            ha = present[(torch.arange(M) * 3) % len(present)]
            hlp = hd.log_prob(ha)
            hi_e = dict(action=ha)
        old, old_v, adv, ret = perturb(hlp, hv, 11 + len(agent))
        hi_e.update(log_prob=old, value=old_v, advantage=adv, returnn=ret)
        counts = branch_counts(hlp, hv, hi_e, ZG_HYPER["clip_eps"])
        if kind != "goal":
            counts["skills_without_a_sample"] = N_SKILLS - len(set(ha.tolist()))
        store_counts(rec, f"{agent}_hi_update", counts)
    for item, e, xs in ((f"{agent}_lo_update", lo_e, dict(obs=lo_obs, zone_obs=lo_zone, **extra)),
                        (f"{agent}_hi_update", hi_e, dict(obs=hi_obs, zone_obs=hi_zone))):
        for k, a in {**xs, **e}.items():
            rec.both(item, f"exp/{k}", np_of(a))
        for k, a in ZG_HYPER.items():
            rec.both(item, f"hyper/{k}", np.float64(a))
        rec.both(item, "shape/NT", np.array([N, T], np.int64))
    torch.set_default_dtype(dtype)
    hi.to(dtype), lo.to(dtype)
    algo = make_algo(T)
    algo.num_frames_lo, algo.num_frames_hi = n, M
    lo_exps = torch_ac.DictList({k: a.to(dtype) for k, a in lo_e.items()})
    lo_exps.obs = widen(lo_x, dtype)
    hi_exps = torch_ac.DictList({k: widen(a, dtype) for k, a in hi_e.items()})
    hi_exps.obs = torch_ac.DictList({"obs": hi_obs.to(dtype), "zone_obs": hi_zone.to(dtype)})
    for item, update, opt, model, fn in (
            (f"{agent}_hi_update", algo.update_hi_parameters, algo.hi_optimizer, hi, "_get_batches_starting_indexes_hi"),
            (f"{agent}_lo_update", algo.update_lo_parameters, algo.lo_optimizer, lo, "_get_batches_starting_indexes_lo")):
        seed_all(80 + len(item))
        lists = []
        undo = wrap_logs(lists)
        try:
            drive_update(rec, item, lambda: update((lo_exps, hi_exps)), opt, model, algo, fn, full=False)
        finally:
            undo()
        names = ("entropy", "value", "policy_loss", "value_loss", "grad_norm")
        assert len(lists) == len(names), (item, len(lists))
        for name, values in zip(names, lists):
            rec.mine(item, f"log/{name}", np.array(values, np.float64))
    return algo, hi_e


def wait_env(spaces, Z, F):
    """The reference's own WaitWrapper around a toy environment: what the skill-family algorithms insist on."""
    from envs.wrappers import WaitWrapper
    return WaitWrapper(ToyEnv(spaces, 0, Z, F, ()))


def widening(spaces, Z, F, dtype):
    from utils.format import get_obss_preprocessor
    _, pre = get_obss_preprocessor(spaces_for(spaces, Z, F)[0])
    return lambda o, device=None: widen(pre(o, device), dtype)


def diayn_updates(rec, algo, inverse, hi_e, Z, F, dtype):
    """update_inverse_parameters on an experience of the recorder's, and two update_skill_prior steps on the high
    level's recorded skills (ABSENT_SKILL never among them)."""
    import torch
    import torch_ac
    item = "inverse_update"
    n = 40
    obs, zone_obs = random_obs(n, Z, F, 90)
    skill = torch.tensor([k for k in range(N_SKILLS) if k != ABSENT_SKILL])[(torch.arange(n) * 3) % (N_SKILLS - 1)]
    rec.both(item, "exp/obs", np_of(obs))
    rec.both(item, "exp/zone_obs", np_of(zone_obs))
    rec.both(item, "exp/skill", np_of(skill))
    rec.both(item, "hyper/lr", np.float64(algo.inverse_lr))
    rec.both(item, "hyper/optim_eps", np.float64(algo.optim_eps))
    store_counts(rec, item, {"skills_without_a_sample": N_SKILLS - len(set(skill.tolist()))})
    exps = torch_ac.DictList({"skill": skill})
    exps.obs = torch_ac.DictList({"obs": obs.to(dtype), "zone_obs": zone_obs.to(dtype)})
    seed_all(91)
    lists = []
    undo = wrap_logs(lists)
    try:
        drive_update(rec, item, lambda: algo.update_inverse_parameters((None, None, exps)), algo.inverse_optimizer,
                     inverse, algo, "_get_batches_starting_indexes_inverse", full=False)
    finally:
        undo()
    assert len(lists) == 1
    rec.mine(item, "log/loss", np.array(lists[0], np.float64))
    item = "prior_update"
    actions = hi_e["action"]
    rec.both(item, "actions", np_of(actions))
    rec.both(item, "hyper/lr", np.float64(1e-2))
    rec.both(item, "hyper/optim_eps", np.float64(algo.optim_eps))
    rec.mine(item, "logits0", np_of(algo.skill_logits))
    hi_exps = torch_ac.DictList({"action": actions})
    for step in (1, 2):
        logs = algo.update_skill_prior((None, hi_exps))
        rec.mine(item, f"logits{step}", np_of(algo.skill_logits))
        rec.mine(item, f"probs{step}", np.array([logs[str(i)] for i in range(N_SKILLS)], np.float64))
    store_counts(rec, item, {"skills_without_a_sample": N_SKILLS - len(set(actions.tolist()))})


def child_xy_goals(rec, spaces, dtype):
    import torch
    from hier_policy_value_models import HighPolicyValueModel, LoPolicyValueModel
    Z, F = CM
    seed_all(4)
    obs_space, action_space = spaces_for(spaces, Z, F)
    shapes = {k: v.shape for k, v in obs_space.spaces.items()}
    hi = HighPolicyValueModel(dict(shapes), H)
    lo = LoPolicyValueModel(dict(shapes), action_space, H)
    g = torch.Generator().manual_seed(SEED + 44)
    goal = torch.rand((B_NET, 2), generator=g, dtype=torch.float32) * 2.0 - 1.0
    two_level_networks(rec, "xy_goals", hi, lo, Z, F, {"goal": goal}, dtype)
    import torch_ac
    h = ZG_HYPER

    def make_algo(T):
        return torch_ac.algos.HierPolicyAlgo([wait_env(spaces, Z, F)], hi, lo, torch.device("cpu"),
                                             widening(spaces, Z, F, dtype), 1, 20, T, h["lr"], h["gae_lambda"],
                                             h["entropy_coef"], h["discount"], h["value_loss_coef"], h["clip_eps"], 1, 10,
                                             h["hi_entropy_coef"], h["hi_value_coef"], h["hi_lr"], h["max_grad_norm"],
                                             h["optim_eps"], 2)

    def algo_for(envs, T, L):
        return torch_ac.algos.HierPolicyAlgo(envs, hi, lo, torch.device("cpu"), widening(spaces, Z, F, dtype), 1, 20, T,
                                             h["lr"], h["gae_lambda"], h["entropy_coef"], h["discount"],
                                             h["value_loss_coef"], h["clip_eps"], 1, 10, h["hi_entropy_coef"],
                                             h["hi_value_coef"], h["hi_lr"], h["max_grad_norm"], h["optim_eps"], L)

    xy_collect(rec, spaces, algo_for, hi, lo, dtype)
    two_level_updates(rec, spaces, "xy_goals", hi, lo, Z, F, dtype, "goal", make_algo)


def skill_family_networks(rec, spaces, agent, ZF, dtype):
    import torch
    from hier_policy_value_models import HighPolicyValueModel, LoPolicyValueModel
    Z, F = ZF
    obs_space, action_space = spaces_for(spaces, Z, F)
    shapes = {k: v.shape for k, v in obs_space.spaces.items()}
    shapes["skill"] = (1,)
    hi = HighPolicyValueModel({k: v for k, v in shapes.items() if k != "skill"}, N_SKILLS, H)
    lo = LoPolicyValueModel(dict(shapes), action_space, N_SKILLS, H)
    skill = torch.arange(B_NET) % N_SKILLS
    two_level_networks(rec, agent, hi, lo, Z, F, {"skill": skill}, dtype, hi_raw=hi.actor.discrete_)
    rec.both(agent, "in/n_skills", np.int64(N_SKILLS))
    return hi, lo


def child_options(rec, spaces, dtype):
    import torch
    import torch_ac
    seed_all(5)
    Z, F = CM
    hi, lo = skill_family_networks(rec, spaces, "options", CM, dtype)
    h = ZG_HYPER

    def make_algo(T):
        return torch_ac.algos.HierPolicyAlgo([wait_env(spaces, Z, F)], hi, lo, torch.device("cpu"),
                                             widening(spaces, Z, F, dtype), True, True, 1, 20, T, h["lr"],
                                             h["gae_lambda"], h["entropy_coef"], h["discount"], h["value_loss_coef"],
                                             h["clip_eps"], 1, 10, h["hi_entropy_coef"], h["hi_value_coef"], h["hi_lr"],
                                             h["max_grad_norm"], h["optim_eps"], N_SKILLS)

    def algo_for(envs, T):
        return torch_ac.algos.HierPolicyAlgo(envs, hi, lo, torch.device("cpu"), widening(spaces, Z, F, dtype), True, True,
                                             1, 20, T, h["lr"], h["gae_lambda"], h["entropy_coef"], h["discount"],
                                             h["value_loss_coef"], h["clip_eps"], 1, 10, h["hi_entropy_coef"],
                                             h["hi_value_coef"], h["hi_lr"], h["max_grad_norm"], h["optim_eps"], N_SKILLS)

    options_collect(rec, spaces, algo_for, hi, dtype)
    two_level_updates(rec, spaces, "options", hi, lo, Z, F, dtype, "option", make_algo)


def inverse_network(rec, spaces, dtype):
    import torch
    import torch_ac
    from inverse_model import InverseModel
    Z, F = TSP
    seed_all(6)
    torch.set_default_dtype(torch.float32)
    model = InverseModel({"obs": (8,), "zone_obs": (Z, F)}, N_SKILLS, H)
    randomise_biases(model, 60)
    for k, v in state_dict_np(model).items():
        rec.both("inverse", f"sd/{k}", v)
    obs, zone_obs = random_obs(B_NET, Z, F, 60)
    rec.both("inverse", "in/obs", np_of(obs))
    rec.both("inverse", "in/zone_obs", np_of(zone_obs))
    rec.both("inverse", "in/n_skills", np.int64(N_SKILLS))
    torch.set_default_dtype(dtype)
    model.to(dtype)
    with torch.no_grad():
        logits = model(torch_ac.DictList({"obs": obs.to(dtype), "zone_obs": zone_obs.to(dtype)}))
    rec.mine("inverse", "out/logits", np_of(logits))
    return model


def child_main(rec, spaces, dtype):
    models = flat_networks(rec, spaces, dtype)
    flat_update(rec, spaces, models, dtype)
    flat_collect(rec, spaces, models, dtype)
    import torch
    torch.set_default_dtype(torch.float32)
    seed_all(7)
    hi, lo = skill_family_networks(rec, spaces, "skills", TSP, dtype)
    inverse = inverse_network(rec, spaces, dtype)
    import torch_ac
    Z, F = TSP
    h = ZG_HYPER
    logits0 = 0.3 * torch.randn(N_SKILLS, generator=torch.Generator().manual_seed(SEED + 8), dtype=torch.float32)

    def make_algo(T):
        return torch_ac.algos.HierPolicyAlgo([wait_env(spaces, Z, F)], hi, lo, inverse, logits0.to(dtype),
                                             torch.device("cpu"), widening(spaces, Z, F, dtype), True, True, 1, 20, T,
                                             h["lr"], h["gae_lambda"], h["entropy_coef"], h["discount"],
                                             h["value_loss_coef"], 0.1, h["clip_eps"], 1, 10, h["hi_entropy_coef"],
                                             h["hi_value_coef"], h["hi_lr"], 1, 16, 3e-4, h["max_grad_norm"],
                                             h["optim_eps"], 2, N_SKILLS)

    def algo_for(envs, T, L):
        return torch_ac.algos.HierPolicyAlgo(envs, hi, lo, inverse, logits0.to(dtype).clone(),
                                             torch.device("cpu"), widening(spaces, Z, F, dtype), True, True, 1, 20, T,
                                             h["lr"], h["gae_lambda"], h["entropy_coef"], h["discount"],
                                             h["value_loss_coef"], 0.1, h["clip_eps"], 1, 10, h["hi_entropy_coef"],
                                             h["hi_value_coef"], h["hi_lr"], 1, 16, 3e-4, h["max_grad_norm"],
                                             h["optim_eps"], L, N_SKILLS)

    skills_collect(rec, spaces, algo_for, hi, lo, dtype)

    algo, hi_e = two_level_updates(rec, spaces, "skills", hi, lo, Z, F, dtype, "skill", make_algo)
    diayn_updates(rec, algo, inverse, hi_e, Z, F, dtype)


# ------------------------------------------------------------------------------------------------ the children and the files
CHILDREN = {"main": child_main, "zone-goals": child_zone_goals, "xy-goals": child_xy_goals, "options": child_options}
PARTS = {"main": {"flat_plain": "networks", "flat_dist": "networks", "flat_plain_update": "flat_update",
                  "flat_dist_update": "flat_update", "flat_collect": "flat_collect", "skills": "skill_networks", "inverse": "skill_networks", "skills_hi_update": "skill_updates",
                  "skills_lo_update": "skill_updates", "inverse_update": "skill_updates", "prior_update": "skill_updates", "skills_collect": "skill_collect"},
         "zone-goals": {"zone_goals": "networks", "zone_goals_hi_update": "hi_update", "zone_goals_lo_update": "lo_update", "zone_goals_collect": "collect"},
         "xy-goals": {"xy_goals": "networks", "xy_goals_hi_update": "updates", "xy_goals_lo_update": "updates", "xy_goals_collect": "collect"},
         "options": {"options": "networks", "options_hi_update": "updates", "options_lo_update": "updates", "options_collect": "collect"}}


def run_child(variant, prec, path):
    import torch
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    spaces = enter_variant(variant)
    rec = Recorder(prec)
    CHILDREN[variant](rec, spaces, torch.float32 if prec == "f32" else torch.float64)
    with open(path, "wb") as f:
        pickle.dump(rec.out, f)
    import multiprocessing
    for worker in multiprocessing.active_children():  # the reference's ParallelEnv leaves its workers to __del__
        worker.terminate()
    sys.stdout.flush()
    os._exit(0)


def pack(arrays):
    """name -> array as one flat buffer per dtype plus a JSON index [name, dtype, shape, offset]: an .npz entry costs a
    few hundred bytes, which two thousand small arrays cannot afford.  tests/agent_goldens.py's load() undoes it."""
    import json
    buffers, index = {}, []
    for name, a in arrays.items():
        a = np.asarray(a)
        flat = buffers.setdefault(a.dtype.str, [])
        index.append([name, a.dtype.str, list(a.shape), int(sum(x.size for x in flat))])
        flat.append(a.reshape(-1))
    out = {"buffer" + dt: np.concatenate(parts) for dt, parts in buffers.items()}
    out["index"] = np.array(json.dumps(index))
    return out


def tree_listing(root):
    return sorted(os.path.join(d, f) for d, _, files in os.walk(root) for f in files)


def main():
    before = tree_listing(REFERENCE)
    total = 0
    for variant in VARIANTS:
        if variant not in CHILDREN:
            continue
        merged = {}
        with tempfile.TemporaryDirectory() as tmp:
            for prec in ("f32", "f64"):
                path = os.path.join(tmp, f"{variant}_{prec}.pkl")
                env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="0")
                subprocess.run([sys.executable, "-B", os.path.abspath(__file__), "--child", variant, prec, path],
                               check=True, env=env)
                with open(path, "rb") as f:
                    out = pickle.load(f)
                for k, v in out.items():
                    if k in merged:                           # what both precisions share must be the same
                        assert merged[k].dtype == v.dtype and np.array_equal(merged[k], v), k
                    merged[k] = v
        files = {}
        for k, v in merged.items():
            item = k.split("/", 1)[0]
            files.setdefault(PARTS[variant][item], {})[k] = v
        for part, arrays in files.items():
            path = os.path.join(HERE, f"agent_{variant}_{part}.npz")
            np.savez_compressed(path, **pack({k: arrays[k] for k in sorted(arrays)}))
            size = os.path.getsize(path)
            total += size
            print(f"wrote {os.path.relpath(path)}: {len(arrays)} arrays, {size} bytes")
            assert size < LIMIT_FILE, (path, size)
    assert total < LIMIT_ALL, total
    assert tree_listing(REFERENCE) == before, "the reference tree changed"
    print(f"{total} bytes in all; the reference tree is as it was")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        run_child(*sys.argv[2:5])
    else:
        main()
