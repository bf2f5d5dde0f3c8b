"""CPU: tests/diayn_update_ref.py against what it restates -- the inverse model's forward (tests/skill_collect_ref.py),
autograd, the reference's kept-sample loops and the prior's loss."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from tests import diayn_update_ref as R
from tests.skill_collect_ref import inverse_log_softmax, random_inverse_state_dict

F64 = torch.float64


def _inputs(B, Zn, F, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal((B, 8)).astype(np.float32), (g.random((B, Zn, F)) * 2 - 1).astype(np.float32)


@pytest.mark.parametrize("F,S,h,Zn", [(6, 5, 32, 4), (7, 1, 31, 1), (6, 32, 33, 3)])
def test_inverse_ref_is_the_inverse_forward(F, S, h, Zn):
    sd = random_inverse_state_dict(F, S, h=h, seed=3)
    obs, zo = _inputs(9, Zn, F, 1)
    for dt, tol in ((torch.float32, 2e-6), (F64, 1e-12)):
        model = R.model_from(sd, F, dt)
        assert [k for k, _ in model.named_parameters()] == list(sd)
        with torch.no_grad():
            logits = model(torch.as_tensor(obs).to(dt), torch.as_tensor(zo).to(dt))
        got = torch.log_softmax(logits, dim=-1).numpy()
        np.testing.assert_allclose(got, inverse_log_softmax(sd, obs, zo, dt), rtol=0, atol=tol)


@pytest.mark.parametrize("S", [1, 2, 5, 32])
def test_numpy_dlogit_and_loss_are_autograd(S):
    g = np.random.default_rng(S)
    skill = g.integers(0, S, 17)
    for dt, tol in ((np.float64, 1e-15), (np.float32, 2e-7)):
        logits = (3 * g.standard_normal((17, S))).astype(dt)
        t = torch.as_tensor(logits).requires_grad_(True)
        loss = F_.cross_entropy(t, torch.as_tensor(skill))
        loss.backward()
        np.testing.assert_allclose(R.dlogit(logits, skill), t.grad.numpy(), rtol=0, atol=tol)
        rows = F_.cross_entropy(t.detach(), torch.as_tensor(skill), reduction="none").numpy()
        np.testing.assert_allclose(R.loss_rows(logits, skill), rows, rtol=0, atol=20 * tol)
    if S == 1:
        assert np.all(R.dlogit(logits, skill) == 0) and np.all(R.loss_rows(logits, skill) == 0)


def test_kept_list_is_the_references_loops():
    N, T = 5, 9
    mask = np.ones((N, T), np.float32)
    mask[0, 0] = 0                  # frame 0 is never a sample's next frame
    mask[1, 1] = 0
    mask[2, T - 1] = 0
    mask[3, 3:7] = 0                # a whole idle window
    mask[4, :] = 0                  # an env that idled throughout
    kept = R.kept_samples(mask)
    np.testing.assert_array_equal(kept, R.kept_samples_loops(mask))
    assert kept.dtype == np.int32 and np.all(np.diff(kept) > 0)
    T1 = T - 1
    assert 0 * T1 + 0 in kept                         # mask[0, 0] does not matter
    assert 1 * T1 + 0 not in kept and 2 * T1 + (T - 2) not in kept
    assert not set(range(3 * T1 + 2, 3 * T1 + 6)) & set(kept.tolist())
    assert not set(range(4 * T1, 5 * T1)) & set(kept.tolist())
    assert len(kept) == N * T1 - 1 - 1 - 4 - T1
    from combinatorial_rl_tasks_amd import agents
    np.testing.assert_array_equal(agents.diayn_kept_samples(mask), kept)
    np.testing.assert_array_equal(R.kept_samples(np.zeros((3, 4))), np.zeros(0, np.int32))
    np.testing.assert_array_equal(R.kept_samples(np.ones((3, 4))), np.arange(9))


def test_batch_pairs_the_next_observation_with_the_skill():
    N, T, Zn, F = 3, 5, 2, 6
    g = np.random.default_rng(0)
    lo = {"obs": g.standard_normal((N, T, 8)), "zone_obs": g.standard_normal((N, T, Zn, F)),
          "skill": g.integers(0, 4, (N, T))}
    idx = np.array([0, 5, 11])
    b = R.batch(lo, idx, F64)
    for k, i in enumerate(idx):
        env, f = i // (T - 1), i % (T - 1)
        np.testing.assert_array_equal(b["obs"][k].numpy(), lo["obs"][env, f + 1])
        np.testing.assert_array_equal(b["zone_obs"][k].numpy(), lo["zone_obs"][env, f + 1])
        assert int(b["skill"][k]) == lo["skill"][env, f]


@pytest.mark.parametrize("S", [1, 5, 32])
def test_prior_gradient_and_step_are_autograd(S):
    g = np.random.default_rng(7 + S)
    logits = g.standard_normal(S)
    actions = g.integers(0, S, 40)
    t = torch.as_tensor(logits).requires_grad_(True)
    F_.cross_entropy(t.expand(40, S), torch.as_tensor(actions)).backward()
    np.testing.assert_allclose(R.prior_gradient(logits, actions, S), t.grad.numpy(), rtol=0, atol=1e-15)
    if S == 1:
        assert R.prior_gradient(logits, actions, S)[0] == 0
    ref = R.PriorRef(logits, F64)
    p, m, v = logits.copy(), np.zeros(S), np.zeros(S)
    for step in range(1, 4):
        want = ref.step(actions)
        R.prior_step_numpy(p, m, v, actions, step)
        np.testing.assert_allclose(p, want, rtol=0, atol=1e-12)
