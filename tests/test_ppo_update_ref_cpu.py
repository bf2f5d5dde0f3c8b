"""CPU: the restated PPO update (tests/ppo_update_ref.py) against torch's own Adam and clip, its index generator against
the rule, and the condition the GPU test of the clipped branches stands on."""
import numpy as np
import pytest
import torch

from tests import ppo_update_ref as R


def test_restated_adam_matches_torch_adam_over_five_steps():
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn((7, 5), generator=g, dtype=torch.float64)
    grads = [torch.randn((7, 5), generator=g, dtype=torch.float64) * 10.0 ** (k - 2) for k in range(5)]
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], 3e-4, eps=1e-8, foreach=False)
    mine, m, v = p0.numpy().copy(), np.zeros((7, 5)), np.zeros((7, 5))
    for step, gr in enumerate(grads, 1):
        p.grad = gr.clone()
        opt.step()
        R.adam_step(mine, gr.numpy(), m, v, step, 3e-4, 1e-8)
        np.testing.assert_allclose(mine, p.detach().numpy(), rtol=0, atol=1e-15)
        st = opt.state[p]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-14, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-14, atol=0)
    assert np.abs(mine - p0.numpy()).max() > 1e-4          # the steps moved something


@pytest.mark.parametrize("scale", [1e-3, 50.0])
def test_restated_clip_matches_clip_grad_norm(scale):
    g = torch.Generator().manual_seed(4)
    ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in ((3, 4), (4,), (1, 4))]
    for p in ps:
        p.grad = scale * torch.randn(p.shape, generator=g, dtype=torch.float64)
    before = [p.grad.clone() for p in ps]
    norm = R.total_norm(before)
    got = torch.nn.utils.clip_grad_norm_(ps, 0.5, foreach=False)
    assert abs(float(got) - norm) <= 1e-12 * norm
    coef = R.clip_coef(norm, 0.5)
    assert (coef == 1.0) == (scale < 1.0)
    for p, b in zip(ps, before):
        np.testing.assert_allclose(p.grad.numpy(), coef * b.numpy(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("batch_num", [0, 1, 2, 3])
@pytest.mark.parametrize("N,batch", [(5, 3), (6, 4), (7, 16)])
def test_index_generator_follows_the_rule(zenv_mod, T, batch_num, N, batch):
    from combinatorial_rl_tasks_amd import agents
    total, recurrence = N * T, 1
    # the rule, literally: arange with step recurrence, permuted; one time in two the starts whose sub-batch would run
    # over the end of a rollout are dropped and the rest shifted by recurrence // 2
    want = np.random.default_rng(9).permutation(np.arange(0, total, recurrence))
    if batch_num % 2 == 1:
        want = want[(want + recurrence) % T != 0]
        want = want + recurrence // 2
    for fn in (R.batch_indexes, agents.ppo_batch_indexes):
        got = fn(total, T, batch_num, np.random.default_rng(9))
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
    if batch_num % 2 == 1:
        assert len(want) == total - N          # T = 1: nothing is left, the reference's quirk
    batches = [want[i:i + batch] for i in range(0, len(want), batch)]
    assert sum(len(b) for b in batches) == len(want) and all(len(b) == batch for b in batches[:-1])


@pytest.mark.parametrize("F,Z,h", [(6, 15, 185), (7, 6, 64), (7, 6, 7)])
def test_perturbed_parameters_reach_the_clipped_branches(F, Z, h):
    """theta + 0.05 N(0, 1) |theta| with the fixed seed moves at least 10 % of 384 synthetic samples onto each side's
    clipped policy branch and 10 % onto the clipped value branch (clip_eps = PERTURB_CLIP_EPS): what
    test_gpu_ppo_update.py's perturbed case relies on to exercise the zero gradients."""
    sd = R.random_state_dict(F, h)
    exps = R.synthetic_experience(sd, F, Z, 24, 16)
    model = R.model_from(R.perturbed(sd), F, torch.float64)
    b = R.as_batch(exps, np.arange(384), torch.float64)
    m_hi, m_lo, m_val = R.branches(model, b, R.PERTURB_CLIP_EPS)
    hi, lo, val = (float(x.double().mean()) for x in (m_hi, m_lo, m_val))
    print(f"clipped: ratio above {hi:.3f}, below {lo:.3f}, value {val:.3f}")
    assert hi >= 0.10 and lo >= 0.10 and val >= 0.10
    assert R.PERTURB_SCALE == 0.05
    # and those samples carry no policy gradient: the loss of the clipped samples alone is flat in the actor
    clipped = torch.nonzero(m_hi | m_lo).squeeze(1).numpy()
    grads, _ = R.gradients(model, R.as_batch(exps, clipped, torch.float64),
                           dict(R.HYPER, clip_eps=R.PERTURB_CLIP_EPS, entropy_coef=0.0, value_loss_coef=0.0))
    assert all(float(g.abs().max()) == 0.0 for k, g in grads.items() if k.startswith("actor."))
