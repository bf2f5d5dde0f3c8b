"""CPU: the learners' public surface against its recorded listing (tests/learner_surface.json): every ppo_* / a2c_* /
hppo_* / xyppo_* / skppo_* / opppo_* / diayn_* method of ``ZoneVecEnv`` and ``TorchZoneEnv`` with its signature and
whether it has a docstring, and every learner entry of ``_native._PROTOTYPES`` / ``_A2C_PROTOTYPES`` with its restype
and argtypes by type name.  The methods and the prototypes are generated from one table of learner families; the
listing was recorded while each was still written out by hand, with

    import json
    from tests.test_learner_surface_cpu import listing
    json.dump(listing(), open("tests/learner_surface.json", "w"), indent=1, sort_keys=True)

No name may be missing and no name may be new."""
import inspect
import json
import os

PREFIXES = ("ppo_", "a2c_", "hppo_", "xyppo_", "skppo_", "opppo_", "diayn_")
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "learner_surface.json")


def listing():
    from combinatorial_rl_tasks_amd import _native as nat
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    from combinatorial_rl_tasks_amd.vec_env import ZoneVecEnv
    out = {}
    for cls in (ZoneVecEnv, TorchZoneEnv):
        out[cls.__name__] = {name: {"signature": str(inspect.signature(f)), "docstring": bool(f.__doc__)}
                             for name, f in inspect.getmembers(cls, inspect.isfunction) if name.startswith(PREFIXES)}
    for table in ("_PROTOTYPES", "_A2C_PROTOTYPES"):
        out[table] = {name: {"restype": restype.__name__, "argtypes": [a.__name__ for a in argtypes]}
                      for name, (restype, argtypes) in getattr(nat, table).items()
                      if name.startswith(tuple("zenv_" + p for p in PREFIXES))}
    return out


def test_learner_surface_is_the_recorded_one():
    with open(RECORD) as f:
        want = json.load(f)
    got = listing()
    assert sorted(got) == sorted(want)
    for section in want:
        assert sorted(got[section]) == sorted(want[section]), section
        for name in want[section]:
            assert got[section][name] == want[section][name], (section, name)
    assert got == want
