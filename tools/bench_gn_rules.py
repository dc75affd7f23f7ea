#!/usr/bin/env python3
"""What an assignment rule behind the GN-model admission check costs (include/orlg.h orlg_step_rule_gn): NSFNET-320,
load 50, +6 dBm per 50 GHz, B = 4096, 1000 steps per launch -- gated sap_ff and sap_ff_gn (the kernels of DESIGN 2.20 / 2.21) and
sap_bf, sap_lf, sap_mc under gn_rule "check" and "next_path", one handle each, in ONE run, the handles alternating so that they
share whatever else the machine does.  Prints one JSON line: env-steps/s of each (median of the repeats, and their spread), the
kernel each ran, the accepted share, the share of steps with more than one check (from the query, over a few single steps), and
the time of one path_rule_windows call next to action_masks("path_ff_gn") (pageable host buffers, copy and wait included).
usage: python tools/bench_gn_rules.py [--batch B] [--steps K] [--repeats R]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

RULE_OF = {"sap_bf": "best", "sap_lf": "last", "sap_mc": "min_cut"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000, help="steps per launch")
    ap.add_argument("--warmup", type=int, default=2, help="launches before the timed ones")
    ap.add_argument("--repeats", type=int, default=5, help="timed launches per handle")
    ap.add_argument("--load", type=float, default=50)
    ap.add_argument("--probe", type=int, default=40, help="single steps that count the checks of a step")
    args = ap.parse_args()
    import numpy as np
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, rmsa_gn_gate_parameters
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    kw = dict(num_spectrum_resources=320, load=args.load, mean_service_holding_time=25, episode_length=1000, seed=10)
    gate = rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0)
    variants = [("sap_ff", "sap_ff", None), ("sap_ff_gn", "sap_ff_gn", None)]
    variants += [(f"{name}:{mode}", name, mode) for name in RULE_OF for mode in ("check", "next_path")]
    envs = {label: BatchedRMSAEnv(topo, args.batch, gn_gate=gate, **kw) for label, _, _ in variants}

    def launch(label, policy, mode, n=args.steps, **more):
        r = envs[label].run(policy, n, auto_reset=True, **(more if mode is None else dict(more, gn_rule=mode)))
        envs[label].synchronize()
        return r

    for _ in range(args.warmup):
        for v in variants:
            launch(*v)
    times = {label: [] for label in envs}
    for _ in range(args.repeats):
        for v in variants:
            t0 = time.perf_counter()
            launch(*v)
            times[v[0]].append(time.perf_counter() - t0)
    out = {"metric": f"env steps/s, RMSA NSFNET-320 load {args.load:g}, +6 dBm, assignment rules behind the GN-model admission check",
           "batch": args.batch, "steps_per_launch": args.steps, "repeats": args.repeats}
    work = args.batch * args.steps
    S, K = kw["num_spectrum_resources"], topo.k_paths
    for label, policy, mode in variants:
        env = envs[label]
        out[label] = {"value": work / statistics.median(times[label]), "min": work / max(times[label]), "max": work / min(times[label]),
                      "kernel": env.last_kernel(), "mean_running": float(env.num_running().mean())}
        r = launch(label, policy, mode, n=min(args.steps, 200), outputs=("gn_gsnr_db", "accepted"))
        checked = np.isfinite(r["gn_gsnr_db"])
        out[label].update(share_accepted=float((r["accepted"] != 0).mean()), share_checked=float(checked.mean()),
                          share_rejected=float((checked & (r["accepted"] == 0)).mean()))
        # the checks of a step, from the query in front of single steps: one under "check"; under "next_path" the paths that have
        # a window up to the first admitted one (all of them where none is admitted)
        rule = "first" if mode is None else RULE_OF[policy]
        many = []
        for _ in range(args.probe):
            slots, _, adm = env.path_rule_windows(rule)
            has = slots < S
            first = np.where(adm.any(axis=1), adm.argmax(axis=1), K)
            checks = (has & (np.arange(K)[None, :] <= first[:, None])).sum(axis=1)
            many.append((checks > 1).mean() if mode == "next_path" or policy == "sap_ff_gn" else 0.0)
            launch(label, policy, mode, n=1)
        out[label]["share_steps_with_more_than_one_check"] = float(np.mean(many))
    # the query next to the path_ff_gn mask, on the handle of sap_bf:check
    env = envs["sap_bf:check"]
    bufs = (np.zeros((args.batch, K), np.int16), np.zeros((args.batch, K)), np.zeros((args.batch, K), np.uint8))
    mask, mg = np.zeros(env.action_mask_shape("path_ff_gn")[0], np.uint8), np.zeros((args.batch, K))
    calls = {"path_ff_gn": lambda: env.action_masks("path_ff_gn", out=mask, gsnr_out=mg)}
    calls.update({f"path_rule_windows:{rule}": (lambda rule=rule: env.path_rule_windows(rule, *bufs)) for rule in ("first", "best", "last", "min_cut")})
    qt = {name: [] for name in calls}
    for i in range(args.warmup + args.repeats):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            env.synchronize()
            if i >= args.warmup:
                qt[name].append(time.perf_counter() - t0)
    out["query_ms_per_call"] = {name: 1e3 * statistics.median(v) for name, v in qt.items()}
    print(json.dumps(out))
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
