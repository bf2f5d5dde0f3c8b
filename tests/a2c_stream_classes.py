"""The stream classes of the A2C learner's entry points (zenv_a2c_*), in the terms of tests/stream_stall.py: what
tests/test_gpu_a2c_update.py's stall test holds each call to, and what tests/test_a2c_update_ref_cpu.py keeps complete
against ``_native._A2C_PROTOTYPES``."""
from tests.stream_stall import ASYNC, HOST_ARG, NO_DEVICE, WAITS

CLASSES = {
    "zenv_a2c_check": (NO_DEVICE, "validates its arguments on the host"),
    "zenv_a2c_tensor": (NO_DEVICE, "hands out an address or a size; the memory is not touched"),
    "zenv_a2c_get_step": (NO_DEVICE, "the host's count of RMSprop steps ENQUEUED so far"),
    "zenv_a2c_set_step": (NO_DEVICE, "the host's count of RMSprop steps ENQUEUED so far"),
    "zenv_a2c_apply": (ASYNC, ""),
    "zenv_a2c_update": (ASYNC, "once the index list of that N T exists: the first call of a size uploads it and waits"),
    "zenv_a2c_accumulate": (HOST_ARG, "idx with idx_on_device == 0"),
    "zenv_a2c_init": (WAITS, ""),
    "zenv_a2c_read": (WAITS, ""),
    "zenv_a2c_write": (WAITS, ""),
}
