#!/usr/bin/env python3
"""Load sweep as ONE handle against the same sweep as one handle per load, run one after another.

    python tools/bench_sweep.py [--kind rmsa|phy] [--loads L0 L1 STEP | --load-list ...] [--seeds N] [--steps K] [--defrag]
                                [--only one|sequential] [--runs R] [--out profiles/sweep.json]

Defaults: RMSA NSFNET-320 sap_ff, 16 loads 20 .. 95 Erlang x 4096 seeds = 65 536 environments, 1000-step launches, warm.
``--kind phy``: QoT-aware US14 bmfa, the reference's seven loads 1200 .. 1680 (tests/test_rmsa_threads_us.py:57-60) x 585 seeds.
The sequential side uses the scalar ``load=`` constructors only, so ``--only sequential`` runs on a build without sweeps.
Timed with HIP events on the handle's stream (torch.cuda.Event on a stream handed to the handles); no counters in the run.
Prints one JSON line and merges it into ``--out`` under its configuration's key; each side records the commit it ran at
(``--commit`` where the tree is not a git checkout)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="rmsa", choices=["rmsa", "phy"])
    ap.add_argument("--load-list", type=float, nargs="+", default=None)
    ap.add_argument("--seeds", type=int, default=None, help="seeds per load (rmsa 4096, phy 585)")
    ap.add_argument("--steps", type=int, default=1000, help="steps per launch")
    ap.add_argument("--launches", type=int, default=3, help="timed launches per run")
    ap.add_argument("--warmup", type=int, default=2, help="warm-up launches")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--defrag", action="store_true", help="phy: defrag_period=10, number_moves=10")
    ap.add_argument("--only", default=None, choices=["one", "sequential"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep.json"))
    ap.add_argument("--commit", default=None, help="commit of the tree this runs in, recorded per side (default: git rev-parse HEAD)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from conftest import load_phy_tables, load_topology
    from optical_rl_gym_amd import BatchedPhyRMSAEnv, BatchedRMSAEnv

    if args.kind == "rmsa":
        loads = args.load_list or [20.0 + 5.0 * i for i in range(16)]
        seeds, policy = args.seeds or 4096, "sap_ff"
        topo = load_topology("nsfnet_chen_5-paths_6-modulations")
        kw = dict(num_spectrum_resources=320, mean_service_holding_time=25, episode_length=1000)

        def make(batch, **traffic):
            return BatchedRMSAEnv(topo, batch, **kw, **traffic)
    else:
        loads = args.load_list or [float(x) for x in range(1200, 1701, 80)]
        seeds, policy = args.seeds or 585, "bmfa"
        topo = load_topology("us14_3-paths_6-modulations")
        pairs, mod, gsnr = load_phy_tables("us14_k3")
        kw = dict(modulation_level=mod, connections_detail=pairs, gsnr=gsnr, mean_service_holding_time=25, episode_length=200,
                  defrag_period=10 if args.defrag else None, number_moves=10 if args.defrag else None)

        def make(batch, **traffic):
            return BatchedPhyRMSAEnv(topo, batch, **kw, **traffic)
    B = len(loads) * seeds
    commit = args.commit
    if commit is None:
        import subprocess
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown"

    def shape(kernel):
        """launch shape from a last_kernel() string: waves per workgroup, LDS bytes per workgroup and how many such workgroups
        the 160 KiB of LDS of a CU hold (the LDS bound on resident waves per CU)"""
        import re
        m = re.search(r"block=(\d+) lds=(\d+)", kernel)
        if not m:
            return None
        waves, lds = int(m.group(1)) // 64, int(m.group(2))
        return {"waves_per_workgroup": waves, "lds_bytes_per_workgroup": lds, "lds_bound_waves_per_cu": (160 * 1024 // lds) * waves}
    stream = torch.cuda.Stream()
    base_seeds = np.arange(seeds, dtype=np.uint64) + np.uint64(10)

    def timed(envs):
        """ms of `launches` launches of every handle, one handle after another on one stream"""
        for e in envs:
            e.set_stream(stream.cuda_stream)
        for _ in range(args.warmup):
            for e in envs:
                e.run(policy, args.steps, auto_reset=True)
        stream.synchronize()
        out = []
        for _ in range(args.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for e in envs:
                for _ in range(args.launches):
                    e.run(policy, args.steps, auto_reset=True)
            t1.record(stream)
            t1.synchronize()
            out.append(t0.elapsed_time(t1))
        for e in envs:
            e.synchronize()     # (reports an overflowed queue)
        return out

    res = {"kind": args.kind, "policy": policy, "loads": loads, "seeds_per_load": seeds, "batch": B, "steps": args.steps,
           "launches": args.launches, "defrag": bool(args.defrag)}
    total = B * args.steps * args.launches
    if args.only != "sequential":
        one = make(B, load=np.repeat(np.asarray(loads), seeds), seeds=np.tile(base_seeds, len(loads)),
                   groups=np.repeat(np.arange(len(loads), dtype=np.int32), seeds), num_groups=len(loads))
        ms = timed([one])
        res["one_handle"] = {"ms": ms, "env_steps_per_s": [total / (m * 1e-3) for m in ms], "kernel": one.last_kernel(),
                             "launch_shape": shape(one.last_kernel()), "commit": commit}
        one.close()
    if args.only != "one":
        envs = [make(seeds, load=ld, seeds=base_seeds) for ld in loads]
        ms = timed(envs)
        res["sequential_handles"] = {"ms": ms, "env_steps_per_s": [total / (m * 1e-3) for m in ms],
                                     "kernels": sorted({e.last_kernel() for e in envs}),
                                     "launch_shape": shape(envs[-1].last_kernel()), "commit": commit}
        for e in envs:
            e.close()
    print(json.dumps(res))
    if args.out:
        key = f"{args.kind}{'_defrag' if args.defrag else ''}_{len(loads)}x{seeds}"
        try:
            doc = json.load(open(args.out))
        except (OSError, ValueError):
            doc = {}
        doc.setdefault(key, {}).update(res)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
