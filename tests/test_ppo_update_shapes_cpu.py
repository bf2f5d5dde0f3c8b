"""CPU: the table of edge shapes (tests/ppo_update_shapes.py) before the GPU tests stand on it.  For every row the float64
and float32 references run on synthetic experience of the row's shape with the row's parameters: every gradient tensor
of the float64 run has a non-zero maximum, so check_rule has a scale to measure against (the high level's actor.2.bias
is exactly zero by construction), the float32 run is finite, and the parameters built for one loss branch put every
sample on it.  The edge columns of the table are the sizes the host code derives (32-row tiles, 256-row chunks)."""
import numpy as np
import pytest
import torch

from tests import hppo_update_ref as RH
from tests import ppo_update_ref as R
from tests import ppo_update_shapes as S

F32, F64 = torch.float32, torch.float64
HIER_T = 33


def _scales(g64, g32, skip=()):
    for k, g in g64.items():
        assert float(g.abs().max()) > 0 or k in skip, k
        assert bool(torch.isfinite(g32[k]).all()), k
    for k in skip:
        assert float(g64[k].abs().max()) < 1e-15, k


@pytest.mark.parametrize("case", list(S.FLAT))
def test_flat_rows_have_a_scale_in_every_gradient(case):
    row = S.FLAT[case]
    sd = S.flat_state_dict(case)
    exps = R.synthetic_experience(sd, row["F"], row["Z"], row["N"], row["T"], seed=row["seed"])
    total = row["N"] * row["T"]
    assert max(row["batches"]) <= total
    for batch in row["batches"]:
        idx = S.batch_indexes(total, batch)
        assert len(idx) == batch and total - 1 in idx
        g = {dt: R.gradients(R.model_from(sd, row["F"], dt), R.as_batch(exps, idx, dt), R.HYPER) for dt in (F64, F32)}
        assert len(g[F64][0]) == (20 if row["dist"] else 18)
        _scales(g[F64][0], g[F32][0])
        assert g[F64][1]["grad_norm"] > 0 and np.isfinite(g[F32][1]["grad_norm"])
        if (case, batch) in S.FLAT_EDGES:
            assert S.edge_of(batch, row["Z"])[:3] == S.FLAT_EDGES[case, batch]
    assert all(k in S.FLAT_EDGES for k in ((c, b) for c in ("z1", "z2", "z32", "h1", "h128", "h128d")
                                           for b in S.FLAT[c]["batches"]))


def test_the_single_unit_of_h1_is_active_in_every_layer():
    row = S.FLAT["h1"]
    sd = S.flat_state_dict("h1")
    exps = R.synthetic_experience(sd, row["F"], row["Z"], row["N"], row["T"], seed=row["seed"])
    b = R.as_batch(exps, np.arange(row["N"] * row["T"]), F64)
    active = S.relu_activity(R.model_from(sd, row["F"], F64), b["obs"], b["zone_obs"])
    print(active)
    assert len(active) == 4 and all(frac > 0 for _, frac in active)      # zone_net_.0, .2, actor.enc_, critic.0


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_sigma_bias_puts_every_sample_on_one_softplus_end(sign):
    row = S.FLAT["h128d"]
    sd = S.flat_state_dict("h128d")
    exps = R.synthetic_experience(sd, row["F"], row["Z"], row["N"], row["T"], seed=row["seed"])
    b = R.as_batch(exps, np.arange(row["N"] * row["T"]), F64)
    learner = S.with_sigma_bias(sd, sign * S.SIGMA_BIAS)
    bx = S.sigma_input(R.model_from(learner, row["F"], F64), b)
    assert bool((bx > 20).all()) if sign > 0 else bool((bx < -20).all())
    # the other 19 tensors are the acting network's: mu, std and the value, hence the ratio of 1, are unchanged
    assert all(torch.equal(learner[k], sd[k]) for k in sd if k != "critic_sigma.bias")
    g = {dt: R.gradients(R.model_from(learner, row["F"], dt), R.as_batch(exps, np.arange(64), dt), R.HYPER)
         for dt in (F64, F32)}
    _scales(g[F64][0], g[F32][0])


def test_saturated_heads_on_every_sample():
    row = S.FLAT["sat"]
    sd = S.flat_state_dict("sat")
    assert sd["actor.mu_.bias"].tolist() == [8.0, -8.0] and sd["actor.std_.bias"].tolist() == [-8.0, 8.0]
    exps = R.synthetic_experience(sd, row["F"], row["Z"], row["N"], row["T"], seed=row["seed"])
    b = R.as_batch(exps, np.arange(row["N"] * row["T"]), F64)
    assert S.heads_saturated(R.model_from(sd, row["F"], F64), b)


@pytest.mark.parametrize("case", list(S.HIER))
def test_zone_goals_rows_have_a_scale_in_every_gradient(case):
    row = S.HIER[case]
    hi_sd, lo_sd = S.hier_state_dicts(case)
    M = 2 * row["N"]                                       # the least a collect of these handles closes
    lo, hi = RH.synthetic_hier_experience(hi_sd, lo_sd, row["F"], row["Z"], row["N"], HIER_T, M, seed=row["seed"])
    for level, sd, exps, total, hyper in (("lo", lo_sd, lo, row["N"] * (HIER_T - 1), RH.LO_HYPER),
                                          ("hi", hi_sd, hi, M, RH.HI_HYPER)):
        for batch in row[level]:
            n = total if batch == "all" else batch
            assert n <= total
            idx = np.arange(total) if batch == "all" else S.batch_indexes(total, n)
            g = {}
            for dt in (F64, F32):
                b = RH.lo_batch(exps, idx, dt) if level == "lo" else RH.hi_batch(exps, idx, dt)
                g[dt] = RH.gradients(level, RH.model_from(level, sd, row["F"], dt), b, hyper)
            assert len(g[F64][0]) == (16 if level == "hi" else 18)
            _scales(g[F64][0], g[F32][0], skip=("actor.2.bias",) if level == "hi" else ())
            if (case, level, n) in S.HIER_EDGES:
                rows, row_chunks, _, split = S.edge_of(n, row["Z"])
                assert (rows, row_chunks, split) == S.HIER_EDGES[case, level, n]
    if case == "bigM":
        assert M >= 320 and S.edge_of(M, row["Z"])[2] == 2          # two sample chunks; k_ppo_stats strides past 256
        assert all((case, lv, n) in S.HIER_EDGES for lv in ("lo", "hi") for n in row[lv] if n != "all")
