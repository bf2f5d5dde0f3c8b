"""zenv_render (csrc/render.hip, K18): the device frames against tests/render_ref.py on the observations fetched with
zenv_get -- byte for byte, no tolerance and no excluded pixel: both sides do the same float32 operations in the same
order (the build has contraction off).  Every task, the sizes and destinations at which the store path changes (fewer
bytes than one 16-byte store, row bytes that are no multiple of 4 or 16, an unaligned base), counts and offsets across
more than one workgroup, idle envs, marks, the torch surface, the experience film and the single-env facade."""
import ctypes as C

import numpy as np
import pytest

from tests import render_ref as R

pytestmark = pytest.mark.gpu


def _env(Z, cfg, n, seed0=500, order=False, goals=False, **over):
    if isinstance(cfg, str):
        cfg = Z.config_for_id(cfg, **over)
    env = Z.ZoneVecEnv(cfg, n)
    if order:
        env.enable_order()
    env.build_bank(seed0, max(n, 3))
    env.schedule_sequential()
    if goals:
        env.enable_goals()
    env.reset()
    return env


def _greedy(Z, env, steps, auto_reset=True):
    for _ in range(steps):
        env.policy(Z.POLICY_GREEDY)
        env.step(None, auto_reset=auto_reset)


def _expect(env, first, count, marks=None, obs=None, **cfg):
    """render_ref of envs first .. first + count - 1 on the handle's current observations (or on obs = (o, zo))."""
    o, zo = env.observations() if obs is None else obs
    rz = R.zone_radius_of(env.cfg.zones_size)
    return np.stack([R.render_ref(o[first + k], zo[first + k], env.cfg.task, rz,
                                  mark=None if marks is None else marks[k], cfg=cfg) for k in range(count)])


def _same(got, want, tag=""):
    assert got.dtype == np.uint8 and got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        raise AssertionError(f"{tag}: {len(bad)} pixels differ, first at (image, row, column) {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])].tolist()} != {want[tuple(bad[0])].tolist()}")


@pytest.mark.parametrize("env_id", ["PointTSP-v0", "PointTSP-v1", "PointTTSP-v0", "ColourMatch-v0", "PointTSP-v4"])
def test_every_task_after_reset_and_after_steps(zenv_mod, env_id):
    Z = zenv_mod
    n = 6
    env = _env(Z, env_id, n)
    _same(env.render(), _expect(env, 0, n), "reset")
    _greedy(Z, env, 40)
    want = _expect(env, 0, n)
    _same(env.render(), want, "after 40 steps")
    assert len({tuple(p) for p in want.reshape(-1, 3)}) >= 4          # background, a zone colour, body, nose
    if env_id == "PointTSP-v4":                                      # some zones start visited: two zone colours at reset
        assert (want == (255, 255, 0)).all(-1).any() and (want == (0, 255, 255)).all(-1).any()
    env.close()


def test_timed_tsp_fade_is_drawn(zenv_mod):
    """Stepped until some unvisited zone's t < 0.5: its disc is neither cyan nor red, and equals the reference."""
    Z = zenv_mod
    env = _env(Z, "PointTTSP-v0", 8, num_steps=400)
    rs = np.random.RandomState(0)
    for _ in range(200):                    # t = (deadline - steps) / num_steps falls by 1 / 400 per step
        env.step(rs.uniform(-0.2, 0.2, (8, 2)).astype(np.float32), auto_reset=True)
        o, zo = env.observations()
        unvisited = (zo[..., 2] == 0) & (zo[..., 3] == 1) & (zo[..., 4] == 1) & (zo[..., 5] != 0)
        if (unvisited & (zo[..., 6] < 0.5) & (zo[..., 6] > 0.05)).any():
            break
    assert (unvisited & (zo[..., 6] < 0.5) & (zo[..., 6] > 0.05)).any(), "no deadline got near"
    got = env.render(width=128, height=128)
    _same(got, _expect(env, 0, 8, obs=(o, zo), width=128, height=128), "fade")
    faded = (got[..., 0] >= 128) & (got[..., 0] < 255) & (got[..., 1] == got[..., 2]) & (got[..., 1] <= 128) & (got[..., 1] > 0)
    assert faded.any()
    env.close()


def _goal_marks(Z, env, zo):
    """What "auto" rings where ZENV_F_GOAL >= 0: that zone's centre / 3 as the observation has it."""
    goal = env.get(Z._native.F_GOAL)
    return np.array([zo[i, g, :2] if g >= 0 else (np.nan, np.nan) for i, g in enumerate(goal)], np.float32)


def test_order_feature_handles(zenv_mod):
    """PointTSP-v2: the vector handle with the route feature switched on, and the facade whose rows have F = 7.  Such a
    handle keeps the next city of its route in ZENV_F_GOAL: "auto" rings it."""
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import envs
    env = _env(Z, "PointTSP-v0", 5, order=True)
    _greedy(Z, env, 40)
    o, zo = env.observations()
    marks = _goal_marks(Z, env, zo)
    assert np.isfinite(marks).any()
    _same(env.render(), _expect(env, 0, 5, marks=marks, obs=(o, zo)), "order handle")
    _same(env.render(marks=None), _expect(env, 0, 5, obs=(o, zo)), "order handle, no marks")
    env.close()
    single = envs.make("PointTSP-v2")
    single.seed(31)
    obs = single.reset()
    for _ in range(40):
        obs = single.step(np.array([0.6, 0.3], np.float32))[0]
    o, zo = _from_dict(obs, single.num_cities)
    assert zo.shape[1] == 7
    want = R.render_ref(o, zo, 0, R.zone_radius_of(0.2), mark=_goal_marks(Z, single._vec, zo[None])[0])
    _same(single.render(), want, "PointTSP-v2 facade")
    single.close()


def _from_dict(obs, zones):
    o = np.concatenate([obs["remaining"], obs["robot_pos"], obs["robot_dir"], obs["robot_velp"], obs["robot_velr"]])
    return o.astype(np.float32), np.stack([obs[f"zones_lidar_{i}"] for i in range(zones)]).astype(np.float32)


@pytest.fixture(scope="module")
def stepped(zenv_mod):
    """One PointTSP-v0 handle of 70 envs after 25 greedy steps, shared (read-only) by the shape tests."""
    Z = zenv_mod
    env = _env(Z, "PointTSP-v0", 70)
    _greedy(Z, env, 25)
    yield env, env.observations()
    env.close()


@pytest.mark.parametrize("width,height", [(1, 1), (3, 5), (17, 9), (64, 64), (100, 100), (129, 31)])
def test_sizes(zenv_mod, stepped, width, height):
    """1 x 1 and 3 x 5 are shorter than one 16-byte store; 17 and 129 columns give row bytes that are no multiple of 4;
    64 x 64 and 100 x 100 are all 16-byte chunks; 17 x 9 (459 bytes) and 129 x 31 (11 997 bytes) start every image at
    another offset from a 16-byte boundary."""
    env, obs = stepped
    got = env.render(first=2, count=5, width=width, height=height, view=1.1, robot_radius=0.25)
    _same(got, _expect(env, 2, 5, obs=obs, width=width, height=height, view=1.1, robot_radius=0.25), f"{width}x{height}")


@pytest.mark.parametrize("count", [1, 2, 63, 65])
def test_counts_and_offsets_ending_at_the_last_env(zenv_mod, stepped, count):
    env, obs = stepped
    first = 70 - count
    got = env.render(first=first, count=count, width=21, height=13)
    _same(got, _expect(env, first, count, obs=obs, width=21, height=13), f"count {count}")
    if count == 65:
        assert np.array_equal(env.render(first=first, width=21, height=13), got)       # count None: to the last env


def test_a_large_frame_spans_workgroups(zenv_mod, stepped):
    """300 x 220 x 3 = 198 000 bytes: 13 workgroups of 16 KiB per image, the last one partly filled."""
    env, obs = stepped
    got = env.render(first=68, count=2, width=300, height=220, view=0.8)
    _same(got, _expect(env, 68, 2, obs=obs, width=300, height=220, view=0.8), "300x220")


def test_single_env_handle(zenv_mod):
    Z = zenv_mod
    env = _env(Z, "ColourMatch-v0", 1)
    _greedy(Z, env, 10)
    _same(env.render(width=40, height=40), _expect(env, 0, 1, width=40, height=40), "N = 1")
    env.close()


@pytest.mark.parametrize("zones", [1, 8, 9, 25])
def test_zone_counts(zenv_mod, zones):
    Z = zenv_mod
    cfg = Z.default_config(Z.TASK_COLOUR_MATCH if zones == 9 else Z.TASK_TSP, zones, zones_keepout=0.3)
    env = _env(Z, cfg, 4)
    _greedy(Z, env, 12)
    _same(env.render(width=90, height=70), _expect(env, 0, 4, width=90, height=70), f"Z = {zones}")
    env.close()


def test_idle_env_draws_background_and_a_noseless_robot_then_comes_back(zenv_mod):
    Z = zenv_mod
    env = _env(Z, "PointTSP-v1", 3, num_steps=6)
    _greedy(Z, env, 8, auto_reset=False)                 # the episodes end at step 6: two no-op steps after that
    o, zo = env.observations()
    assert not o.any() and not zo.any()
    got = env.render()
    _same(got, _expect(env, 0, 3, obs=(o, zo)), "idle")
    assert {tuple(p) for p in got.reshape(-1, 3)} == {R.BACKGROUND, R.BODY}
    r, c = np.argwhere((got[0] == R.BODY).all(-1)).mean(0)
    assert abs(r - 49.5) <= 0.5 and abs(c - 49.5) <= 0.5               # the disc sits on the origin
    _greedy(Z, env, 1, auto_reset=True)
    back = env.render()
    _same(back, _expect(env, 0, 3), "after the auto-reset")
    assert (back == (0, 255, 255)).all(-1).any()
    env.close()


def test_marks(zenv_mod, stepped):
    env, obs = stepped
    kw = dict(width=80, height=80)
    assert np.array_equal(env.render(first=10, count=4, marks=None, **kw), env.render(first=10, count=4, **kw))   # "auto": none here
    marks = np.array([[0.3, -0.2], [np.nan, 0.1], [-0.9, 0.9], [0.0, np.nan]], np.float32)
    got = env.render(first=10, count=4, marks=marks, **kw)
    _same(got, _expect(env, 10, 4, marks=marks, obs=obs, **kw), "explicit marks")
    ringed = [(img == R.MARK).all(-1).any() for img in got]
    assert ringed == [True, False, True, False]
    with pytest.raises(ValueError):
        env.render(first=10, count=4, marks=marks[:3], **kw)


def test_auto_marks_on_a_goal_conditioned_handle(zenv_mod):
    Z = zenv_mod
    n = 5
    env = _env(Z, "PointTSP-v0", n, goals=True)             # PointTSP-v3
    before = env.render(width=120, height=120)
    _same(before, _expect(env, 0, n, width=120, height=120), "no goal yet")
    assert not (before == R.MARK).all(-1).any()
    goals = np.array([3, -1, 0, 14, 7], np.int32)
    env.set_goals(goals)
    o, zo = env.observations()
    marks = np.array([zo[i, g, :2] if g >= 0 else (np.nan, np.nan) for i, g in enumerate(goals)], np.float32)
    got = env.render(width=120, height=120)
    _same(got, _expect(env, 0, n, marks=marks, obs=(o, zo), width=120, height=120), "auto marks")
    assert [(img == R.MARK).all(-1).any() for img in got] == [True, False, True, True, True]
    _same(env.render(first=2, count=3, width=120, height=120), got[2:], "auto marks with an offset")
    _same(env.render(width=120, height=120, marks=None), before, "marks=None")
    env.close()


def test_unaligned_and_host_destinations(zenv_mod, stepped):
    """A device dst one byte past an aligned base, and the staged host path, give the aligned device dst's bytes; the
    bytes before and after the frames stay untouched."""
    import torch
    Z = zenv_mod
    env, obs = stepped
    first, count = 7, 3
    for width, height in ((64, 64), (17, 9), (1, 1)):
        nbytes = count * height * width * 3
        want = _expect(env, first, count, obs=obs, width=width, height=height)
        outs = []
        for shift in (0, 1, 5, 15):
            buf = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()                # (the handle draws on its own stream)
            assert buf.data_ptr() % 16 == 0
            env._render(Z.RENDER_CURRENT, 0, first, count, width, height, 1.25, 0.1, None, False,
                        buf.data_ptr() + 16 + shift, True)
            env.sync()
            host = buf.cpu().numpy()
            assert (host[:16 + shift] == 0xAB).all() and (host[16 + shift + nbytes:] == 0xAB).all(), (width, shift)
            outs.append(host[16 + shift:16 + shift + nbytes].reshape(want.shape))
        for shift, got in zip((0, 1, 5, 15), outs):
            _same(got, want, f"{width}x{height} at base + {shift}")
        _same(env.render(first=first, count=count, width=width, height=height), want, "host dst")


def test_torch_surface(zenv_mod):
    import torch
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    Z = zenv_mod
    n = 9
    env = _env(Z, "PointTSP-v0", n, goals=True)
    tenv = TorchZoneEnv(env)
    env.set_goals(np.arange(n, dtype=np.int32) % 4 - 1)
    host = env.render(width=50, height=36)
    out = tenv.render(width=50, height=36)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, 36, 50, 3)
    _same(out.cpu().numpy(), host, "torch vs numpy")
    assert (host == R.MARK).all(-1).any()
    again = tenv.render(first=1, count=n - 1, width=50, height=36, out=out[1:])      # a view: contiguous, unaligned base + 5400
    assert again.data_ptr() == out[1:].data_ptr()
    _same(out.cpu().numpy(), host, "torch out=")
    marks = torch.tensor([[0.1, 0.2], [float("nan"), 0.0]], device="cuda")
    got = tenv.render(first=3, count=2, width=50, height=36, marks=marks)
    _same(got.cpu().numpy(), env.render(first=3, count=2, width=50, height=36, marks=marks.cpu().numpy()), "torch marks")
    with pytest.raises(ValueError):
        tenv.render(width=50, height=36, out=out[:, :, :, :2])
    env.close()


def _raw(Z, env, field, shape):
    a = np.empty(shape, np.float32)
    assert a.nbytes == env.field_bytes(field)
    Z._native.check(Z._native.lib().zenv_get(env._h, field, a.ctypes.data, 0))
    return a


def _expect_film(Z, env, e, T, marks=None, **cfg):
    n = env.num_envs
    o = _raw(Z, env, Z._native.F_EXP_OBS, (T, n, 8))[:, e]
    zo = _raw(Z, env, Z._native.F_EXP_ZONE_OBS, (T, n, env.num_zones, env.zone_feat))[:, e]
    rz = R.zone_radius_of(env.cfg.zones_size)
    return np.stack([R.render_ref(o[t], zo[t], env.cfg.task, rz, mark=None if marks is None else marks[t], cfg=cfg)
                     for t in range(T)])


def test_experience_film_of_the_flat_collector(zenv_mod):
    from oracle import policy_ref as P
    Z = zenv_mod
    n, T = 70, 6
    env = _env(Z, "PointTSP-v1", n, num_steps=4)          # episodes end, and start again, inside the film
    with pytest.raises(Z.ZenvError) as err:
        env.render_experience(69)
    assert err.value.code == Z.E_STATE and "experience" in str(err.value)
    env.load_mlp(P.random_tensors(env.zone_feat, h=64, seed=1, critic=True), precision="f32")
    env.collect(T, policy_seed=3)
    want = _expect_film(Z, env, 69, T, width=60, height=44)
    _same(env.render_experience(69, width=60, height=44), want, "film of env 69")
    _same(env.render_experience(69, first=2, count=3, width=60, height=44), want[2:5], "frames 2 .. 4")
    _same(env.render_experience(0, width=60, height=44), _expect_film(Z, env, 0, T, width=60, height=44), "env 0")
    for first, count in ((0, T + 1), (T, 1), (3, 4)):
        with pytest.raises(Z.ZenvError) as err:
            env.render_experience(69, first=first, count=count)
        assert err.value.code == Z.E_ARG and "first + count" in str(err.value)
    with pytest.raises(Z.ZenvError) as err:
        env.render_experience(70)
    assert err.value.code == Z.E_ARG and "env" in str(err.value)
    # the current observations are still what render() draws
    _same(env.render(first=60, width=60, height=44), _expect(env, 60, 10, width=60, height=44), "current after collect")
    env.close()


def test_experience_film_of_the_hier_collector_with_auto_marks(zenv_mod):
    import torch
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    from tests import hier_ref
    Z = zenv_mod
    n, T = 70, 6
    env = _env(Z, "PointTSP-v1", n, goals=True)
    hi, lo = hier_ref.random_state_dicts(env.zone_feat, h=32, seed=2, critics=True)
    env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
    env.collect_hier(T, policy_seed=5)
    goals = _raw(Z, env, Z._native.F_LO_GOAL, (T, n, 2))[:, 69]
    assert np.isfinite(goals).all()
    want = _expect_film(Z, env, 69, T, marks=goals, width=96, height=96)
    got = env.render_experience(69, width=96, height=96)
    _same(got, want, "hier film, auto marks")
    assert all((img == R.MARK).all(-1).any() for img in got)
    _same(env.render_experience(69, width=96, height=96, marks=None),
          _expect_film(Z, env, 69, T, width=96, height=96), "hier film, no marks")
    tenv = TorchZoneEnv(env)
    film = tenv.render_experience(69, first=1, count=4, width=96, height=96)
    assert film.is_cuda and film.dtype == torch.uint8
    _same(film.cpu().numpy(), want[1:5], "torch film")
    env.close()


def test_never_reset_handle_is_refused(zenv_mod):
    Z = zenv_mod
    env = Z.ZoneVecEnv("PointTSP-v1", 2)
    with pytest.raises(Z.ZenvError) as err:
        env.render()
    assert err.value.code == Z.E_STATE and "reset" in str(err.value)
    dst = np.zeros(2 * 30000, np.uint8)
    rc = Z.RenderConfig(100, 100, Z.RENDER_CURRENT, 0, 1.25, 0.1)
    lib = Z._native.lib()
    assert lib.zenv_render(env._h, C.byref(rc), 0, 2, None, 0, None, 0) == Z.E_ARG
    assert lib.zenv_render(env._h, C.byref(rc), 1, 2, None, 0, dst.ctypes.data, 0) == Z.E_ARG
    assert b"first + count" in lib.zenv_last_error() and not dst.any()
    env.close()


def test_facade_renders_through_the_host_io_slab(zenv_mod):
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import envs
    env = envs.make("PointTSP-v1")
    assert env.metadata["render.modes"] == ["rgb_array"]
    env.seed(12)
    obs = env.reset()
    rz = R.zone_radius_of(0.2)
    first = env.render()
    assert first.shape == (100, 100, 3) and first.dtype == np.uint8
    _same(first, R.render_ref(*_from_dict(obs, env.num_cities), 0, rz), "facade after reset")
    for _ in range(30):
        env.step(np.array([0.9, -0.4], np.float32))
    frame = env.render()
    _same(frame, R.render_ref(*_from_dict(env.obs(), env.num_cities), 0, rz), "facade after steps")
    assert not np.array_equal(frame, first)
    small = env.render(mode="rgb_array", width=33, height=20)
    _same(small, R.render_ref(*_from_dict(env.obs(), env.num_cities), 0, rz, cfg=dict(width=33, height=20)), "33x20")
    with pytest.raises(NotImplementedError):
        env.render(mode="human")
    env.close()
    goal_env = envs.make("PointTSP-v3")
    goal_env.seed(4)
    obs = goal_env.reset()
    goal_env.set_goal(2)
    o, zo = _from_dict(obs, goal_env.num_cities)
    _same(goal_env.render(), R.render_ref(o, zo, 0, rz, mark=zo[2, :2]), "PointTSP-v3 facade rings its goal")
    goal_env.close()


def test_the_same_call_twice_gives_the_same_bytes(zenv_mod, stepped):
    env, _ = stepped
    a = env.render(width=64, height=64)
    b = env.render(width=64, height=64)
    assert np.array_equal(a, b)
    out = np.empty_like(a)
    assert env.render(width=64, height=64, out=out) is out and np.array_equal(out, a)


def test_the_visualize_example_writes_an_animation(zenv_mod, tmp_path):
    """examples/visualize.py, the counterpart of the reference's scripts/visualize.py: one short episode to a file."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "run.gif"
    done = subprocess.run([sys.executable, os.path.join(root, "examples", "visualize.py"), "--env", "PointTSP-v1",
                           "--policy", "greedy", "--episodes", "1", "--max-steps", "40", "--size", "48",
                           "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "Eps len: 40" in done.stdout and "11 frames of 48 x 48" in done.stdout
    try:
        from PIL import Image
    except ImportError:
        frames = np.load(tmp_path / "run.npy")
        assert frames.shape == (11, 48, 48, 3) and frames.dtype == np.uint8
        return
    with Image.open(out) as im:
        assert im.format == "GIF" and im.size == (48, 48) and im.n_frames >= 2
