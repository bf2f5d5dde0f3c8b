"""The head-normalising helpers of tests/xy_ref.py and tests/option_ref.py (scale_head_rows / normalise_heads) on
synthetic observations: at weight scale 3 the sigmoid heads' pre-activations are in the tens to hundreds; afterwards
every |pre-activation - bias| is at most 3, only the head weight rows that needed it have changed, and the float64
outputs are clear of the sigmoid's flat ends.  No device."""
import numpy as np
import pytest
import torch

from tests import option_ref, xy_ref

F64 = torch.float64
HEADS = ("actor.mu_", "actor.std_")
# sigmoid at |x| <= 4: mu = 2 (s - 0.5) within +-0.9641, std = s + 1e-3 within 0.0190 .. 0.9831
MU_MAX, STD_MIN, STD_MAX = 0.9641, 0.0189, 0.9831


def _batch(h, Z, F, B=37):
    rs = np.random.RandomState(h)
    return (rs.uniform(-1, 1, (B, 8)).astype(np.float32), rs.uniform(-1, 1, (B, Z, F)).astype(np.float32),
            rs.uniform(-2, 2, (B, 2)).astype(np.float32), rs)


def _check_dict(sd, before, pre, pre_before):
    """Only head weights moved; each row by one factor >= 1, exactly 1 where the row was within 3 already."""
    for k in before:
        if k in [f"{n}.weight" for n in HEADS]:
            continue
        assert torch.equal(sd[k], before[k]), k
    r = 0
    for n in HEADS:
        w0, w1, b = before[f"{n}.weight"].double(), sd[f"{n}.weight"].double(), sd[f"{n}.bias"].double().numpy()
        assert sd[f"{n}.weight"].dtype == torch.float32
        for i in range(w0.shape[0]):
            over = np.abs(pre_before[:, r] - b[i]).max() / 3.0
            if over <= 1.0:
                assert torch.equal(w0[i], w1[i]), (n, i)
            else:
                assert torch.allclose(w1[i] * over, w0[i], rtol=1e-6, atol=0), (n, i)
            assert np.abs(pre[:, r] - b[i]).max() <= 3.0 * (1 + 1e-6), (n, i)
            r += 1
    assert r == pre.shape[1] and np.abs(pre).max() <= 4.0


def _pre_xy(sd, x, zo):
    a = xy_ref._head_input(sd, x, zo)
    return torch.cat([a @ sd[f"{n}.weight"].double().T + sd[f"{n}.bias"].double() for n in HEADS], dim=1).numpy()


@pytest.mark.parametrize("h", [1, 33, 191])
def test_xy_heads_are_brought_within_range(h):
    F, Z = 6, 9
    obs, zo, goal, rs = _batch(h, Z, F)
    hi, lo = xy_ref.random_state_dicts(F, h, seed=h, weight_scale=3.0)
    has = rs.rand(len(obs)) < 0.6
    x_lo = np.concatenate([obs, goal], axis=1)[has]
    before = [{k: v.clone() for k, v in sd.items()} for sd in (hi, lo)]
    pre0 = _pre_xy(hi, obs, zo), _pre_xy(lo, x_lo, zo[has])
    if h > 1:
        assert max(np.abs(p).max() for p in pre0) > 4.0         # the case needs the helper
    pre_hi, pre_lo = xy_ref.normalise_heads(hi, lo, obs, zo, goal, has)
    assert pre_hi.shape == (len(obs), 4) and pre_lo.shape == (has.sum(), 4) and pre_hi.dtype == np.float64
    # what it returns is what the dicts give now
    assert np.array_equal(pre_hi, _pre_xy(hi, obs, zo)) and np.array_equal(pre_lo, _pre_xy(lo, x_lo, zo[has]))
    _check_dict(hi, before[0], pre_hi, pre0[0])
    _check_dict(lo, before[1], pre_lo, pre0[1])
    for mu, std in (xy_ref.high(hi, obs, zo, dtype=F64)[:2], [a[has] for a in xy_ref.low(lo, obs, zo, goal, dtype=F64)[:2]]):
        assert np.abs(mu).max() <= MU_MAX and std.min() >= STD_MIN and std.max() <= STD_MAX
    # no env with a goal: the low level stays as it is
    keep = {k: v.clone() for k, v in lo.items()}
    _, none = xy_ref.normalise_heads(hi, lo, obs, zo, goal, np.zeros(len(obs), bool))
    assert none.shape == (0, 4) and all(torch.equal(lo[k], keep[k]) for k in keep)


@pytest.mark.parametrize("h", [1, 33, 191])
def test_option_heads_are_brought_within_range(h):
    F, Z, S = 7, 8, 5
    obs, zo, _, rs = _batch(h, Z, F)
    hi, lo = option_ref.random_state_dicts(F, S, h=h, seed=h, weight_scale=3.0)
    assert np.allclose(lo["actor.mu_.weight"].double().pow(2).sum(1).sqrt().numpy(), 3.0)   # the third row too
    skill = np.where(rs.rand(len(obs)) < 0.7, rs.randint(0, S, len(obs)), -1)
    has = skill >= 0
    before = {k: v.clone() for k, v in lo.items()}
    pre = option_ref.normalise_heads(lo, obs, zo, skill, S)
    assert pre.shape == (has.sum(), 6) and np.abs(pre).max() <= 4.0
    for k in before:
        if k not in [f"{n}.weight" for n in HEADS]:
            assert torch.equal(lo[k], before[k]), k
    for n, cols in zip(HEADS, (pre[:, :3], pre[:, 3:])):
        b = lo[f"{n}.bias"].double().numpy()
        assert np.abs(cols - b).max() <= 3.0 * (1 + 1e-6)
        ratio = before[f"{n}.weight"].double() / lo[f"{n}.weight"].double()
        assert (ratio.min(dim=1).values >= 1 - 1e-6).all()
        assert torch.allclose(ratio, ratio[:, :1].expand_as(ratio), rtol=1e-5)       # one factor per row
    mu, std, _ = option_ref.low(lo, obs, zo, np.where(has, skill, 0), S, dtype=F64)
    assert mu.shape[1] == 3
    assert np.abs(mu[has]).max() <= MU_MAX and std[has].min() >= STD_MIN and std[has].max() <= STD_MAX
    # the returned pre-activations are those of the restatement: sigmoid of them gives its outputs
    assert np.allclose(2 * (1 / (1 + np.exp(-pre[:, :3])) - 0.5), mu[has], rtol=0, atol=1e-12)
    assert np.allclose(1 / (1 + np.exp(-pre[:, 3:])) + 1e-3, std[has], rtol=0, atol=1e-12)
    # no env with a skill: nothing changes
    keep = {k: v.clone() for k, v in lo.items()}
    none = option_ref.normalise_heads(lo, obs, zo, np.full(len(obs), -1), S)
    assert none.shape == (0, 6) and all(torch.equal(lo[k], keep[k]) for k in keep)
