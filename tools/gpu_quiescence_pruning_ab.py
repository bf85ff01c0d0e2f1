"""Price list of SPX_SELFPLAY_QUIESCE_PRUNING: the quiescence price list of tools/gpu_quiescence_ab.py repeated with pruning off
and on in one session - the same nets, seeds, seats and game cap, Q in {2, 4, 8} (and Q = 0 once, the yardstick) at node budget
1 000: positions recorded per second, leaf evals/s, nodes per search split into main-search and quiescence nodes, candidates
evaluated per quiescence node. Every setting runs in a process of its own under its own time limit, and the script stops at
the first one that fails.
The synthetic nets know nothing about chess (tools/gpu_quiescence_ab.py): the table prices the option, it does not predict
what a trained net would gain.
Usage: python tools/gpu_quiescence_pruning_ab.py [--seats 4096] [--max-plies 12] [--presets realistic,tame] [--budgets 1000]
       [--plies 2,4,8] [--limit 600]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(args):
    import stormphrax_amd as sp

    preset, budget, q, prune = args.one[0], int(args.one[1]), int(args.one[2]), bool(int(args.one[3]))
    games = args.games or args.seats
    net = sp.Network(sp.synthetic_net_bytes(preset))
    with sp.NnueState(net, device=0, max_batch=args.seats * 64) as st:
        stats = st.selfplay(n_games=args.seats, target_games=games, out_path=None, max_plies=args.max_plies, dfrc=True,
                            temperature_cp=0, seed=1, search_nodes=budget, quiesce_plies=q, quiesce_pruning=prune)
        split = st.selfplay_search_stats()
    sec, moves = stats["seconds"], max(1, stats["positions"])
    per_main = split["main_children"] / max(1, split["main_nodes"])
    per_q = split["quiesce_candidates"] / max(1, split["quiesce_nodes"])
    print(f"{preset:9s} {budget:5d} {q} {'on ' if prune else 'off'} | {stats['positions'] / sec:.4g} | {stats['evals'] / sec:.4g} | "
          f"{stats['steps'] / sec:.4g} | {split['main_nodes'] / moves:.1f} + {split['quiesce_nodes'] / moves:.1f} | {per_main:.1f} | "
          f"{per_q:.2f} | {sec:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seats", type=int, default=4096)
    ap.add_argument("--games", type=int, default=0, help="games to finish per run (0 = the number of seats)")
    ap.add_argument("--max-plies", type=int, default=12)
    ap.add_argument("--presets", default="realistic,tame")
    ap.add_argument("--budgets", default="1000")
    ap.add_argument("--plies", default="2,4,8")
    ap.add_argument("--limit", type=int, default=600, help="seconds one setting may take")
    ap.add_argument("--one", nargs=4, metavar=("PRESET", "BUDGET", "Q", "PRUNE"), help="(internal) run one setting and print its line")
    args = ap.parse_args()
    if args.one:
        return one(args)

    t_start = time.perf_counter()
    print(f"# pruned quiescence price list  {args.seats} seats, {args.games or args.seats} games per run, ply cap {args.max_plies}, "
          f"DFRC openings, seed 1; every line a process of its own")
    print("# preset budget Q pruning | positions/s | leaf evals/s | nodes/s | nodes per move: main + quiescence | "
          "children per main node | candidates per quiescence node | seconds", flush=True)
    for preset in args.presets.split(","):
        for budget in (int(b) for b in args.budgets.split(",")):
            for q, prune in [(0, 0)] + [(int(x), p) for x in args.plies.split(",") for p in (0, 1)]:
                cmd = [sys.executable, os.path.abspath(__file__), "--seats", str(args.seats), "--games", str(args.games),
                       "--max-plies", str(args.max_plies), "--one", preset, str(budget), str(q), str(prune)]
                try:
                    rc = subprocess.run(cmd, timeout=args.limit).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print(f"# {preset} budget {budget} Q {q} pruning {prune}: exit status {rc}; stopping here", flush=True)
                    return rc
    print(f"# wall time {time.perf_counter() - t_start:.1f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
