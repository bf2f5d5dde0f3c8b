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


def hier_hyper(h, level):
    """The recorded hyper/* of a two-level update as the learners of a level ("hi" / "lo") take them.  The reference
    clips at neither level (its clip_grad_norm_ lines are commented out in every variant)."""
    pre = "hi_" if level == "hi" else ""
    return dict(lr=float(h[pre + "lr"]), adam_eps=float(h["optim_eps"]), clip_eps=float(h["clip_eps"]),
                entropy_coef=float(h[pre + "entropy_coef"]),
                value_loss_coef=float(h["hi_value_coef" if level == "hi" else "value_loss_coef"]),
                max_grad_norm=float("inf"))


# ---- the sketch of a large gradient.  The fixtures cannot hold the [h, .] gradients of every learner (1 MiB for all of
# them), so for a gradient G [r, c] of more than SMALL elements that is not stored in full they hold G v and u^T G:
# r + c numbers.  The probes are closed-form (no RNG stream to keep stable), at least 0.5 everywhere and without a
# repeated entry among the first 64.  G v has one entry per row and u^T G one per column, so swapped rows or columns
# move entries of the sketch to other places, a transposed gradient changes both halves, and one wrong element moves two
# entries by at least half its error.  What a sketch cannot see: a disturbance D with D v = 0 and u^T D = 0, an
# (r - 1)(c - 1)-dimensional space no indexing or formula mistake is confined to; the GPU tests therefore also compare
# such gradients element by element with the restatement, which the sketch pins to the reference.
SMALL = 256                                          # elements; make_agent_goldens.drive_update stores up to here in full


def probe_v(c):
    """The right probe v [c]."""
    return np.cos(0.7 * np.arange(c, dtype=np.float64) + 0.3) + 1.5


def probe_u(r):
    """The left probe u [r]."""
    return np.cos(0.7 * np.arange(r, dtype=np.float64) + 1.1) + 1.5


def sketch(g):
    """float64 [r + c]: the concatenation [G v, u^T G] of a gradient G [r, c] of any float dtype, computed in float64
    (a tensor of another rank is read as [shape[0], the rest])."""
    g = np.asarray(g, np.float64)
    g = g.reshape(g.shape[0], -1)
    return np.concatenate([g @ probe_v(g.shape[1]), probe_u(g.shape[0]) @ g])
