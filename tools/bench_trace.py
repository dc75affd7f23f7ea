#!/usr/bin/env python3
"""What replaying a request trace costs or saves against generating the same traffic on the device.

    python tools/bench_trace.py [--steps 1000] [--runs 3] [--out profiles/trace.json]       # the four steps, one after another
    python tools/bench_trace.py --config rmsa|phy --side generated|replay                    # one step

Two configurations: the headline (NSFNET-320, sap_ff, B = 65 536) and US14 bmfa at B = 4096; each once with generated
traffic and once replaying the trace recorded from that same handle (``record_trace``: steps + 1 requests per environment).
Every timed launch starts from a full reset -- which rewinds a trace handle -- so both sides run ``steps`` steps from an empty
network, warm (one untimed launch first), timed with HIP events around the launch alone on the handle's stream.
Without ``--side`` the tool runs the four steps as child processes, each under its own ``timeout``, and stops at the first
that fails.  Prints one JSON line per step and merges it into ``--out`` with the kernel string and the commit."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEP_TIMEOUT_S = {"rmsa": 420, "phy": 240}


def commit_of(tree):
    try:
        return subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def one_step(args):
    import torch
    from conftest import load_phy_tables, load_topology
    from optical_rl_gym_amd import BatchedPhyRMSAEnv, BatchedRMSAEnv, record_trace
    if args.config == "rmsa":
        topo, B, policy = load_topology("nsfnet_chen_5-paths_6-modulations"), args.batch or 65536, "sap_ff"
        kw = dict(num_spectrum_resources=320, episode_length=1000)

        def make(**traffic):
            return BatchedRMSAEnv(topo, B, **kw, **traffic)
    else:
        topo, B, policy = load_topology("us14_3-paths_6-modulations"), args.batch or 4096, "bmfa"
        pairs, mod, gsnr = load_phy_tables("us14_k3")
        kw = dict(modulation_level=mod, connections_detail=pairs, gsnr=gsnr, episode_length=200)

        def make(**traffic):
            return BatchedPhyRMSAEnv(topo, B, **kw, **traffic)
    generated = dict(load=50 if args.config == "rmsa" else 1400, mean_service_holding_time=25, seed=10)
    env = make(**generated)
    if args.side == "replay":
        trace = record_trace(env, policy, args.steps, auto_reset=True)
        trace.outputs = None
        env.close()
        env = make(trace=trace)
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    ms = []
    for i in range(args.runs + 1):   # (the first launch is the warm-up)
        env.reset(only_episode_counters=False)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        env.run(policy, args.steps, auto_reset=True)
        t1.record(stream)
        t1.synchronize()
        if i:
            ms.append(t0.elapsed_time(t1))
    env.synchronize()
    res = {"config": args.config, "side": args.side, "batch": B, "policy": policy, "steps": args.steps, "ms": ms,
           "env_steps_per_s": [B * args.steps / (m * 1e-3) for m in ms], "kernel": env.last_kernel(),
           "trace_bytes_on_device": 20 * B * (args.steps + 1) if args.side == "replay" else 0, "commit": args.commit or commit_of(ROOT)}
    env.close()
    print(json.dumps(res), flush=True)
    if args.out:
        try:
            doc = json.load(open(args.out))
        except (OSError, ValueError):
            doc = {}
        doc.setdefault(args.config, {})[args.side] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["rmsa", "phy"], default=None)
    ap.add_argument("--side", choices=["generated", "replay"], default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace.json"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    if args.side:
        if not args.config:
            ap.error("--side needs --config")
        return one_step(args)
    # the four steps, each a fresh process under its own time limit; the first failure ends the run
    for config in ([args.config] if args.config else ["rmsa", "phy"]):
        for side in ("generated", "replay"):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[config]), sys.executable, os.path.abspath(__file__), "--config", config,
                   "--side", side, "--steps", str(args.steps), "--runs", str(args.runs), "--out", args.out]
            if args.batch:
                cmd += ["--batch", str(args.batch)]
            if args.commit:
                cmd += ["--commit", args.commit]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"bench_trace: {config} / {side} ended with status {rc}; stopping", file=sys.stderr)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
