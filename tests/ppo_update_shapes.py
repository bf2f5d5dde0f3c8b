"""The edge shapes the device learners are tested at: one table for tests/test_ppo_update_shapes_cpu.py (which checks on
synthetic experience that every gradient has a scale and every branch condition holds at these seeds) and for the two
GPU files test_gpu_ppo_update_shapes.py / test_gpu_hppo_update_shapes.py.

Why these: k_ppo_tn reduces kPpoChunk = 256 rows per wave, the products work on 32-row tiles and HP = h rounded up past
the constant column to 32, the Zone-goals learners add more than kPpoReduceSplit = 16 chunk partials with
k_ppo_reduce_split, k_ppo_stats strides over 256 threads, and the config takes 1 .. 32 zones."""
import numpy as np
import torch

from tests import hier_ref as H
from tests import ppo_update_ref as R

CHUNK, TILE, SPLIT = 256, 32, 16      # kPpoChunk, the products' row tile, kPpoReduceSplit (csrc/ppo_update.hpp)

TSP, CM = ("id", "PointTSP-v0"), ("id", "ColourMatch-v0")


def zones(n, **over):
    return ("zones", n, over)


# ---- the flat learner: name -> config, Z, F, h, N envs x T frames, critic, parameter seed, minibatch sizes
FLAT = {
    "z1": dict(cfg=zones(1), Z=1, F=6, h=33, N=12, T=24, dist=False, seed=1, batches=(1, 32, 33, 255, 256, 257, 288)),
    "z2": dict(cfg=zones(2), Z=2, F=6, h=31, N=6, T=8, dist=False, seed=2, batches=(31, 48)),
    "z32": dict(cfg=zones(32, zones_keepout=0.30), Z=32, F=6, h=32, N=4, T=8, dist=False, seed=3, batches=(8, 9, 32)),
    "h1": dict(cfg=TSP, Z=15, F=6, h=1, N=4, T=8, dist=False, seed=3, batches=(32,)),
    "h128": dict(cfg=TSP, Z=15, F=6, h=128, N=8, T=8, dist=False, seed=5, batches=(64,)),
    "h128d": dict(cfg=TSP, Z=15, F=6, h=128, N=8, T=8, dist=True, seed=6, batches=(64,)),
    # the handles of the stale-workspace, dropped-index and saturated-heads tests
    "cm64": dict(cfg=CM, Z=6, F=7, h=64, N=5, T=8, dist=False, seed=7, batches=(5, 33, 37, 40)),
    "sat": dict(cfg=CM, Z=6, F=7, h=64, N=5, T=8, dist=False, seed=8, batches=(40,)),
}
# what makes a minibatch an edge: (case, samples) -> zone rows, row chunks (k_ppo_tn over zone rows), sample chunks
FLAT_EDGES = {
    ("z1", 1): (1, 1, 1), ("z1", 32): (32, 1, 1), ("z1", 33): (33, 1, 1), ("z1", 255): (255, 1, 1),
    ("z1", 256): (256, 1, 1), ("z1", 257): (257, 2, 2), ("z1", 288): (288, 2, 2),
    ("z2", 31): (62, 1, 1), ("z2", 48): (96, 1, 1),
    ("z32", 8): (256, 1, 1), ("z32", 9): (288, 2, 1), ("z32", 32): (1024, 4, 1),
    ("h1", 32): (480, 2, 1), ("h128", 64): (960, 4, 1), ("h128d", 64): (960, 4, 1),
}

# ---- the Zone-goals learners: goal-enabled, 12-step episodes, 33 frames (M >= 2 N); minibatch sizes per level
HIER = {
    "bigM": dict(cfg=zones(16, zones_keepout=0.40), Z=16, F=6, h=33, N=160, seed=1, lo=(256, 257, 1000),
                 hi=(255, 256, 257, "all")),
    "z2": dict(cfg=zones(2), Z=2, F=6, h=31, N=8, seed=2, lo=("all",), hi=("all",)),
    "z32": dict(cfg=zones(32, zones_keepout=0.30), Z=32, F=6, h=32, N=8, seed=3, lo=("all",), hi=("all",)),
    "h128": dict(cfg=TSP, Z=15, F=6, h=128, N=8, seed=4, lo=(100,), hi=("all",)),
    # the stale-workspace test's handle: M >= 40 > 37
    "cm64": dict(cfg=CM, Z=6, F=7, h=64, N=20, seed=5, lo=(5, 37), hi=(5, 37)),
}
# (case, level, samples) -> zone rows, row chunks, whether the zone-row gradients go through k_ppo_reduce_split
HIER_EDGES = {
    ("bigM", "hi", 255): (4080, 16, False), ("bigM", "hi", 256): (4096, 16, False), ("bigM", "hi", 257): (4112, 17, True),
    ("bigM", "lo", 256): (4096, 16, False), ("bigM", "lo", 257): (4112, 17, True), ("bigM", "lo", 1000): (16000, 63, True),
    ("z32", "lo", 256): (8192, 32, True), ("h128", "lo", 100): (1500, 6, False),
}


def make_cfg(Z, spec, **extra):
    """spec: ("id", registry id) or ("zones", n, overrides) for the TSP task with n zones."""
    if spec[0] == "id":
        return Z.config_for_id(spec[1], **extra)
    return Z.default_config(0, spec[1], **dict(spec[2], **extra))


def padded_rows(samples, Z):
    """Zone rows and samples as launch_ppo_minibatch pads them to the 32-row tile."""
    return -(-samples * Z // TILE) * TILE, -(-samples // TILE) * TILE


def chunks(rows):
    return -(-rows // CHUNK)


def edge_of(samples, Z):
    """-> (zone rows, row chunks, sample chunks, split reduce of the zone-row gradients in a Zone-goals learner)"""
    rp, bp = padded_rows(samples, Z)
    return samples * Z, chunks(rp), chunks(bp), chunks(rp) > SPLIT


def batch_indexes(total, batch):
    """The flat tests' minibatch: `batch` of `total` sample indexes, the last valid one among them."""
    idx = np.random.default_rng(batch).permutation(total)[:batch]
    idx[-1] = total - 1
    return idx


# ---- parameters that put every sample on one loss branch
SIGMA_BIAS = 80.0           # critic_sigma.bias = +80: softplus' threshold branch (0.3 x > 20); -80: its far negative end


def with_sigma_bias(sd, value):
    out = {k: v.clone() for k, v in sd.items()}
    out["critic_sigma.bias"] = torch.full_like(out["critic_sigma.bias"], value)
    return out


def saturated(sd):
    """actor.mu_.bias = (+8, -8), actor.std_.bias = (-8, +8): mu near +1 and -1, std near its 1e-3 floor and near 1."""
    out = {k: v.clone() for k, v in sd.items()}
    out["actor.mu_.bias"] = torch.tensor([8.0, -8.0])
    out["actor.std_.bias"] = torch.tensor([-8.0, 8.0])
    return out


def flat_state_dict(case):
    row = FLAT[case]
    sd = R.random_state_dict(row["F"], row["h"], row["dist"], seed=row["seed"])
    return saturated(sd) if case == "sat" else sd


def hier_state_dicts(case):
    row = HIER[case]
    return H.random_state_dicts(row["F"], h=row["h"], seed=row["seed"])


def sigma_input(model, b):
    """0.3 x per sample, x = critic_sigma's output: what softplus(beta = 0.3, threshold 20) branches on."""
    with torch.no_grad():
        Zn = b["zone_obs"].shape[1]
        x = torch.cat([b["obs"].unsqueeze(1).expand(-1, Zn, -1), b["zone_obs"]], dim=-1)
        emb = model.env_model.combine_net_(torch.cat([b["obs"], model.env_model.zone_net_(x).sum(dim=1) / Zn], dim=-1))
        return 0.3 * model.critic_sigma(model.critic(emb)).squeeze(1)


def heads_saturated(model, b):
    """Every sample: mu = (near +1, near -1), std = (near the floor, near 1)."""
    with torch.no_grad():
        mu, std, _, _ = model(b["obs"], b["zone_obs"])
    return bool((mu[:, 0] > 0.9).all() and (mu[:, 1] < -0.9).all() and (std[:, 0] < 0.05).all() and (std[:, 1] > 0.95).all())


def relu_activity(model, *inputs):
    """The fraction of positive outputs of every ReLU of `model` on a forward pass, in module order."""
    out, hooks = [], []
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.ReLU):
            hooks.append(m.register_forward_hook(lambda _m, _i, y, name=name: out.append((name, float((y > 0).double().mean())))))
    with torch.no_grad():
        model(*inputs)
    for hk in hooks:
        hk.remove()
    return out
