"""The stream contract's table (tests/stream_stall.py CLASSES) against the binding's signature table: every entry point
is in exactly one class, nothing unknown is classified, and a new entry point cannot appear without someone deciding
whether it is asynchronous, synchronises, reads caller host memory or never touches a stream.  No GPU."""
import re

from tests import stream_stall as S


def _prototypes():
    from combinatorial_rl_tasks_amd import _native as nat
    return nat._PROTOTYPES


def test_every_entry_point_is_classified_exactly_once():
    names = set(_prototypes())
    missing = sorted(names - set(S.CLASSES))
    assert not missing, f"new entry points without a stream class (tests/stream_stall.py): {missing}"
    unknown = sorted(set(S.CLASSES) - names)
    assert not unknown, f"classified, but not in _native._PROTOTYPES: {unknown}"
    # exactly once: the table's builder refuses a second entry (its assert), and a dict holds a name once; the source
    # must not name a function in two put() lists either, which that assert turns into an import error
    assert len(S.CLASSES) == len(names)


def test_classes_and_reasons():
    for name, (cls, why) in S.CLASSES.items():
        assert cls in (S.ASYNC, S.WAITS, S.HOST_ARG, S.NO_DEVICE), name
        assert isinstance(why, str)
        if cls == S.NO_DEVICE:
            assert why.strip(), f"{name}: a NO_DEVICE entry needs its one-line reason"
        if cls == S.HOST_ARG:
            assert why.strip(), f"{name}: a HOST_ARG entry names the host argument"
    assert S.class_of("zenv_step") == S.HOST_ARG and S.class_of("zenv_policy") == S.ASYNC
    assert S.class_of("zenv_get") == S.WAITS and S.class_of("zenv_version") == S.NO_DEVICE


def test_every_handle_free_function_is_no_device_or_says_why():
    """A function without a handle argument has no stream to be ordered on."""
    import ctypes as C
    for name, (_, argtypes) in _prototypes().items():
        takes_handle = bool(argtypes) and argtypes[0] is C.c_void_p and name not in (
            "zenv_host_free", "zenv_comm_unique_id", "zenv_route_ranks", "zenv_route_ranks_shared")
        if not takes_handle and name != "zenv_create":
            assert S.class_of(name) == S.NO_DEVICE, name


def test_the_header_declares_what_the_table_classifies():
    """The table follows the binding, the binding follows include/zenv.h: every classified name is declared there."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "zenv.h")) as f:
        declared = set(re.findall(r"\b(zenv_[a-z0-9_]+)\s*\(", f.read()))
    assert not sorted(set(S.CLASSES) - declared)


def test_stall_length_is_bounded():
    assert 0 < S.DEFAULT_STALL_MS <= S.MAX_STALL_MS <= 500.0
