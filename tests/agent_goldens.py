"""Reading tests/golden/agent_*.npz (written by tests/golden/make_agent_goldens.py): shared by
tests/test_agent_goldens_cpu.py and tests/test_gpu_agent_goldens.py."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(variant, part):
    """name -> array of one fixture.  The file holds one flat buffer per dtype and a JSON index [name, dtype, shape,
    offset] (make_agent_goldens.pack).  A missing fixture is an error, never a skip."""
    path = os.path.join(GOLDEN, f"agent_{variant}_{part}.npz")
    assert os.path.exists(path), f"missing fixture {path}: run tests/golden/make_agent_goldens.py"
    with np.load(path) as z:
        buffers = {k[len("buffer"):]: z[k] for k in z.files if k.startswith("buffer")}
        index = json.loads(str(z["index"]))
    out = {}
    for name, dt, shape, offset in index:
        size = int(np.prod(shape, dtype=np.int64))
        out[name] = buffers[dt][offset:offset + size].reshape(shape)
    return out


def sub(d, prefix):
    return {k[len(prefix):]: v for k, v in d.items() if k.startswith(prefix)}
