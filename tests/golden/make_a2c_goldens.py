"""Record one ``update_parameters`` of the reference's own ``torch_ac.A2CAlgo`` (recurrence 1) on a recorded batch, as
the fixture of tests/test_a2c_update_ref_cpu.py and tests/test_gpu_a2c_update.py.

Built the way make_agent_goldens.py builds its files and on its helpers (imported by path): the stand-in ``gym``, the toy
environments, fresh child processes started with ``python -B``, one run in float32 and one in float64 on the same
float32 weights and inputs.  Only data is stored; nothing of the reference's text is copied.

Two facts about the reference decide how it can be driven at all:

  * ``a2c.py`` is the same file in all four trees, but in ``main`` and ``options`` ``BaseAlgo.__init__`` takes a
    ``distributional_value`` argument that ``A2CAlgo.__init__`` does not pass: the object cannot be constructed there.  The
    children therefore enter the ``zone-goals`` tree, whose ``BaseAlgo`` matches and whose flat ``ACModel`` is main's plain
    one.
  * ``policy_loss = -(dist.log_prob(sb.action) * sb.advantage).mean()`` (a2c.py:53) multiplies [B, 2] by [B]: with the Box
    policy's two-component Normal it raises for every B but 1 and 2.  ``ppo.py:73-76`` in the same package sums the two
    components' log-probabilities before they meet the advantage, and that is the reading this project's A2C learner
    takes.  So the model handed to ``A2CAlgo`` is wrapped (``SummedLogProb`` below, this project's own code): its
    distribution is the reference's Normal with ``log_prob`` summed over the last dimension; ``entropy()`` stays per
    component, as PPO has it.  Every other statement that runs -- the means, the loss, ``RMSprop``, the norm,
    ``clip_grad_norm_``, the logs -- is the reference's own.

Run (needs the reference tree, by default /root/reference, else $ZENV_REFERENCE):

    python tests/golden/make_a2c_goldens.py            writes tests/golden/agent_main_a2c_update.npz
"""
import importlib.util
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _maker():
    spec = importlib.util.spec_from_file_location("zenv_make_agent_goldens", os.path.join(HERE, "make_agent_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _maker()
TREE = "zone-goals"                                  # see the docstring: main's A2CAlgo cannot be constructed
ITEM = "flat_a2c_update"
NT = (6, 8)                                          # envs x frames: A2C's default frames per proc
A2C_HYPER = dict(lr=0.01, rmsprop_alpha=0.99, rmsprop_eps=1e-8, entropy_coef=0.01, value_loss_coef=0.5,
                 max_grad_norm=0.5)


def child(prec, path):
    import torch
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    spaces = M.enter_variant(TREE)
    import torch_ac
    from flat_model import ACModel
    from utils.format import get_obss_preprocessor
    dtype = torch.float32 if prec == "f32" else torch.float64
    rec = M.Recorder(prec)
    Z, F = M.TSP
    N, T = NT
    n = N * T

    class SummedLogProb(torch.nn.Module):
        """The reference's model with its Normal's log_prob summed over the action's components (ppo.py:73-76)."""
        recurrent = False

        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, obs):
            dist, value = self.inner(obs)

            class Summed(torch.distributions.Normal):
                def log_prob(self, a):
                    return super().log_prob(a).sum(dim=-1)

            return Summed(dist.mean, dist.stddev), value

    M.seed_all(31)
    torch.set_default_dtype(torch.float32)
    obs_space, action_space = M.spaces_for(spaces, Z, F)
    model = ACModel({k: v.shape for k, v in obs_space.spaces.items()}, action_space, M.H)
    M.randomise_biases(model, 31)
    for k, v in M.state_dict_np(model).items():
        rec.both(ITEM, f"sd/{k}", v)
    obs, zone_obs = M.random_obs(n, Z, F, 31)
    e = M.gaussian_experience(lambda: model(torch_ac.DictList({"obs": obs, "zone_obs": zone_obs})), n, 2, 31)
    rec.both(ITEM, "exp/obs", M.np_of(obs))
    rec.both(ITEM, "exp/zone_obs", M.np_of(zone_obs))
    for k, a in e.items():
        rec.both(ITEM, f"exp/{k}", M.np_of(a))
    for k, a in A2C_HYPER.items():
        rec.both(ITEM, f"hyper/{k}", np.float64(a))
    rec.both(ITEM, "shape/NT", np.array([N, T], np.int64))
    torch.set_default_dtype(dtype)
    model = model.to(dtype)
    envs = [M.ToyEnv(spaces, j, Z, F, ()) for j in range(N)]
    _, pre = get_obss_preprocessor(envs[0].observation_space)
    h = A2C_HYPER
    algo = torch_ac.algos.A2CAlgo(envs, SummedLogProb(model), torch.device("cpu"), T, 0.99, h["lr"], 0.95,
                                  h["entropy_coef"], h["value_loss_coef"], h["max_grad_norm"], 1, h["rmsprop_alpha"],
                                  h["rmsprop_eps"], lambda o, device=None: M.widen(pre(o, device), dtype))
    assert list(algo._get_starting_indexes()) == list(range(n))
    exps = torch_ac.DictList({k: a.to(dtype) for k, a in e.items()})
    exps.obs = torch_ac.DictList({"obs": obs.to(dtype), "zone_obs": zone_obs.to(dtype)})
    logs = algo.update_parameters(exps)
    for k, v in logs.items():
        rec.mine(ITEM, f"log/{k}", np.float64(float(v)))
    for name, p in model.named_parameters():
        st = algo.optimizer.state[p]
        rec.mine(ITEM, f"param/{name}", M.np_of(p))
        rec.mine(ITEM, f"square_avg/{name}", M.np_of(st["square_avg"]))
        rec.mine(ITEM, f"step/{name}", np.float64(float(st["step"])))
    with open(path, "wb") as f:
        pickle.dump(rec.out, f)
    import multiprocessing
    for worker in multiprocessing.active_children():
        worker.terminate()
    sys.stdout.flush()
    os._exit(0)


def main():
    before = M.tree_listing(M.REFERENCE)
    merged = {}
    with tempfile.TemporaryDirectory() as tmp:
        for prec in ("f32", "f64"):
            path = os.path.join(tmp, f"a2c_{prec}.pkl")
            env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="0")
            subprocess.run([sys.executable, "-B", os.path.abspath(__file__), "--child", prec, path], check=True, env=env)
            with open(path, "rb") as f:
                out = pickle.load(f)
            for k, v in out.items():
                if k in merged:
                    assert merged[k].dtype == v.dtype and np.array_equal(merged[k], v), k
                merged[k] = v
    path = os.path.join(HERE, "agent_main_a2c_update.npz")
    np.savez_compressed(path, **M.pack({k: merged[k] for k in sorted(merged)}))
    size = os.path.getsize(path)
    print(f"wrote {os.path.relpath(path)}: {len(merged)} arrays, {size} bytes")
    assert size < M.LIMIT_FILE, (path, size)
    assert M.tree_listing(M.REFERENCE) == before, "the reference tree changed"


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:4])
    else:
        main()
