"""What the flat agent on a solver-ordered handle costs (zenv_order_rows, K22 k_order_rows, order_rows.hip).

    python scripts/order_collect_time.py [--quick] [--envs N] [--frames T] [--hidden H] [--out FILE.json]

One process, N = 65 536 envs, the paths taking turns; every figure is a median of 5 timed spans with min and max, and
every span ends in a synchronise.

  rows kernel   k_order_rows alone (zenv_device_ptr(ZENV_F_ORDER_ROWS) enqueues exactly that launch) against a
                device-to-device copy of the same output bytes on the same stream; a span is LAUNCHES launches.  Both
                read and write N * Z * 7 floats, so GB/s counts twice the output bytes for either; the ratio is
                kernel time / copy time.
  collector     zenv_collect per frame on PointTSP-v2 (solver-ordered, order_rows on) against PointTTSP-v0: both have
                15 zones and the same 7-wide network, so the difference is what the order step and the rows kernel
                cost.  A span is one collection of T frames.

--quick shortens the run (a rehearsal, not a measurement).  --out writes the figures as JSON."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
SPANS = 5


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def random_tensors(shapes, seed):
    rs = np.random.RandomState(seed)
    return {k: (rs.standard_normal(s) * (0.1 if "_b" in k else 1.0 / np.sqrt(s[-1]))).astype(np.float32)
            for k, s in shapes.items()}


def summary(ms):
    ms = np.asarray(ms, np.float64)
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max())}


def main():
    sys.path.insert(0, ROOT)
    import torch
    import combinatorial_rl_tasks_amd as Z
    from combinatorial_rl_tasks_amd import agents
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv

    n, T, H = arg("--envs", 4096 if QUICK else 65536), arg("--frames", 4 if QUICK else 16), arg("--hidden", 185)
    launches = 5 if QUICK else 50
    handles = {}
    for env_id in ("PointTSP-v2", "PointTTSP-v0"):
        order = env_id == "PointTSP-v2"
        env = Z.ZoneVecEnv(Z.config_for_id("PointTSP-v0" if order else env_id), n)
        if order:
            env.enable_order()
            env.order_rows()
        env.build_bank(1, 4096, n_threads=16)
        env.schedule_sequential()
        tenv = TorchZoneEnv(env)
        tenv.reset()
        assert env.net_zone_feat == 7 and env.num_zones == 15
        shapes = {k: v for k, v in agents.mlp_tensor_shapes(H, 7).items() if "sigma" not in k}
        env.load_mlp(random_tensors(shapes, 1))
        env.rollout(8, Z.POLICY_MLP_SAMPLE, policy_seed=2)       # off the first observation: routes under way
        handles[env_id] = (env, tenv)

    # ---- the rows kernel beside a copy of the same bytes
    env, tenv = handles["PointTSP-v2"]
    rows = tenv.net_rows
    out_bytes = rows.numel() * 4
    src, dst = torch.empty_like(rows), torch.empty_like(rows)
    src.copy_(rows)

    def span_kernel():
        for _ in range(launches):
            env.device_ptr(Z.F_ORDER_ROWS)

    def span_copy():
        for _ in range(launches):
            dst.copy_(src)

    def timed(fn, per):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / per

    for fn in (span_kernel, span_copy):                              # warm-up
        timed(fn, launches)
    ms = {"kernel": [], "copy": []}
    for _ in range(SPANS):                                           # the paths take turns
        ms["kernel"].append(timed(span_kernel, launches))
        ms["copy"].append(timed(span_copy, launches))
    assert torch.equal(rows, torch.cat([tenv.zone_obs, tenv._alias(Z.F_ORDER_VAL).unsqueeze(-1)], dim=-1))
    result = {"envs": n, "zones": 15, "hidden": H, "frames": T, "spans": SPANS, "launches_per_span": launches,
              "quick": QUICK, "rows_kernel": {"output_bytes": out_bytes}}
    for name in ("kernel", "copy"):
        s = summary(ms[name])
        s["gb_per_s"] = 2 * out_bytes / (s["median"] * 1e-3) / 1e9
        result["rows_kernel"][name + "_ms"] = s
    result["rows_kernel"]["ratio_to_copy"] = (result["rows_kernel"]["kernel_ms"]["median"] /
                                              result["rows_kernel"]["copy_ms"]["median"])

    # ---- the collector, per frame
    def span_collect(env_id, c):
        return lambda: handles[env_id][0].collect_on_device(T, policy_seed=c)

    for env_id in handles:
        timed(span_collect(env_id, 0), T)
    per_frame = {env_id: [] for env_id in handles}
    for c in range(SPANS):
        for env_id in handles:
            per_frame[env_id].append(timed(span_collect(env_id, 1 + c), T))
    result["collector_ms_per_frame"] = {env_id: summary(v) for env_id, v in per_frame.items()}
    a, b = (result["collector_ms_per_frame"][k]["median"] for k in ("PointTSP-v2", "PointTTSP-v0"))
    result["collector_ms_per_frame"]["difference"] = a - b
    result["collector_ms_per_frame"]["ratio"] = a / b

    rk = result["rows_kernel"]
    print(f"{n} envs x 15 zones, hidden {H}; medians of {SPANS} spans (min .. max)")
    for name in ("kernel", "copy"):
        s = rk[name + "_ms"]
        print(f"    rows {name:6s} {s['median'] * 1e3:9.1f} us ({s['min'] * 1e3:.1f} .. {s['max'] * 1e3:.1f}), "
              f"{s['gb_per_s']:.0f} GB/s over 2 x {out_bytes / 1e6:.1f} MB")
    print(f"    k_order_rows / copy = {rk['ratio_to_copy']:.3f}")
    for env_id in handles:
        s = result["collector_ms_per_frame"][env_id]
        print(f"    zenv_collect {env_id:13s} {s['median']:8.3f} ms per frame ({s['min']:.3f} .. {s['max']:.3f})")
    print(f"    difference {a - b:+.3f} ms per frame, ratio {a / b:.3f}", flush=True)
    out = arg("--out", "", str)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    for env, _ in handles.values():
        env.close()


if __name__ == "__main__":
    main()
