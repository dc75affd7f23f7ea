#!/usr/bin/env python3
"""Secondary benchmark: BASELINE.json configs[2] -- QoT-aware RMSA (PhyRMSA) on US14, batch 4096, bmfa(cut) heuristic
on the device.  Prints one JSON line (env steps/s).  usage: python tools/bench_phy.py [--batch B] [--steps K] [--load L]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3000)
    ap.add_argument("--chunk", type=int, default=250)
    ap.add_argument("--load", type=float, default=1400)
    ap.add_argument("--metrics", action="store_true", help="also compute number_cuts_total / rss_total_metric every step")
    ap.add_argument("--policy", default="bmfa", choices=["bmfa", "bmfa_rss", "sapff", "bmff", "sapbm", "faff", "faff_rss"])
    ap.add_argument("--grooming", action="store_true")
    ap.add_argument("--defrag", action="store_true", help="defrag_period=10, number_moves=10 (tests/test_rmsa_threads_us.py:190-251)")
    ap.add_argument("--metric", default="cut")
    ap.add_argument("--moves", type=int, default=10, help="number_moves with --defrag")
    ap.add_argument("--period", type=int, default=10, help="defrag_period with --defrag")
    ap.add_argument("--queue", type=int, default=0, help="queue_capacity (0 = from the load)")
    ap.add_argument("--continuous", type=int, nargs=2, metavar=("LOWER", "HIGHER"), default=None,
                    help='bit_rate_selection="continuous" with rng.randint(LOWER, HIGHER) bit rates (phy_rmsa_env.py:114-129)')
    ap.add_argument("--topology", default="us14_3-paths_6-modulations",
                    help="another fixture (e.g. spn_3-paths_6-modulations: 30 nodes / 56 links, the structural limits of DESIGN 6) runs "
                         "with SYNTHETIC QoT tables (levels 1..6 at random): a timing, not a reference workload")
    args = ap.parse_args()
    import torch
    from conftest import load_phy_tables, load_topology
    from optical_rl_gym_amd import BatchedPhyRMSAEnv
    topo = load_topology(args.topology)
    if args.topology.startswith("us14_3"):
        pairs, mod, gsnr = load_phy_tables("us14_k3")
    else:
        import numpy as np
        rng = np.random.default_rng(5)
        N = topo.num_nodes
        pairs = np.array([(a + 1, b + 1) for a in range(N) for b in range(a + 1, N)], dtype=np.int32)
        mod = rng.integers(1, 7, size=(len(pairs), 268, max(3, topo.k_paths))).astype(np.uint8)
        gsnr = rng.uniform(5.0, 25.0, size=mod.shape)
    env = BatchedPhyRMSAEnv(topo, args.batch, modulation_level=mod, connections_detail=pairs, gsnr=gsnr, load=args.load,
                            mean_service_holding_time=25, episode_length=200, seed=10, grooming=args.grooming,
                            defrag_period=args.period if args.defrag else None, number_moves=args.moves if args.defrag else None,
                            metric=args.metric, queue_capacity=args.queue,
                            **(dict(bit_rate_selection="continuous", bit_rate_lower_bound=args.continuous[0],
                                    bit_rate_higher_bound=args.continuous[1]) if args.continuous else {}))
    outs = ("number_cuts_total", "rss_total_metric") if args.metrics else ()

    def run(k):
        left = k
        while left > 0:
            n = min(left, args.chunk)
            env.run(args.policy, n, auto_reset=True, outputs=outs)
            left -= n
    run(args.warmup)
    env.synchronize(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    env.synchronize(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    red, _ = env.reduce_counters()
    st = env.episode_stats()
    print(json.dumps({"metric": f"env steps/s, PhyRMSA {args.topology} {args.policy}", "kernel": env.last_kernel(), "node_vectors": bool(env.node_vectors), "value": args.batch * args.steps / dt,
                      "grooming": args.grooming, "defrag": args.defrag, "defrag_metric": args.metric,
                      "continuous": args.continuous,
                      "queue_overflow": int(st["queue_overflow"].max()),
                      "batch": args.batch, "steps": args.steps, "load": args.load, "metrics_every_step": args.metrics,
                      "ms_per_step": dt * 1e3 / args.steps, "mean_running": float(env.num_running().mean()),
                      "service_blocking_rate": (red["services_processed"] - red["services_accepted"]) / red["services_processed"]}))
    env.close()


if __name__ == "__main__":
    main()
