"""Price list of SPX_SELFPLAY_QUIESCE_PLIES in one process: the device-resident self-play driver with a live search, the same
seeds for every setting, Q in {0, 2, 4, 8} x node budgets {64, 1000}: leaf evals/s, nodes expanded per second (= seat rounds/s),
expansions per move played split into main-search and quiescence nodes, children evaluated per expansion of each kind, the
candidates' share of the legal moves the generator mode spares (estimated from the main nodes' mean), positions recorded and
games finished per second.
The synthetic nets know nothing about chess: a stand pat cuts little, so the quiescence trees are far wider than a trained
net's would be - the table bounds the cost of the option from above, it does not predict it.
Usage: python tools/gpu_quiescence_ab.py [--seats 4096] [--presets tame,realistic] [--budgets 64,1000] [--plies 0,2,4,8]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rocm_version():
    try:
        return open("/opt/rocm/.info/version").read().strip()
    except OSError:
        return subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()[0:1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seats", type=int, default=4096)
    ap.add_argument("--games", type=int, default=0, help="games to finish per run (0 = the number of seats)")
    ap.add_argument("--max-plies", type=int, default=60)
    ap.add_argument("--presets", default="tame,realistic")
    ap.add_argument("--budgets", default="64,1000")
    ap.add_argument("--plies", default="0,2,4,8")
    args = ap.parse_args()

    import torch

    import stormphrax_amd as sp

    games = args.games or args.seats
    t_start = time.perf_counter()
    print(f"# quiescence price list  rocm {rocm_version()}  torch {torch.__version__}  {args.seats} seats, {games} games per run, "
          f"ply cap {args.max_plies}, DFRC openings, seed 1")
    print("# preset budget Q | leaf evals/s | nodes/s | positions/s | games/s | nodes per move: main + quiescence | "
          "children per main node | candidates per quiescence node (share of the main nodes' mean) | seconds")
    for preset in args.presets.split(","):
        net = sp.Network(sp.synthetic_net_bytes(preset))
        for budget in (int(b) for b in args.budgets.split(",")):
            for q in (int(x) for x in args.plies.split(",")):
                with sp.NnueState(net, device=0, max_batch=args.seats * 64) as st:
                    stats = st.selfplay(n_games=args.seats, target_games=games, out_path=None, max_plies=args.max_plies, dfrc=True,
                                        temperature_cp=0, seed=1, search_nodes=budget, quiesce_plies=q)
                    split = st.selfplay_search_stats()
                sec, moves = stats["seconds"], max(1, stats["positions"])
                per_main = split["main_children"] / max(1, split["main_nodes"])
                per_q = split["quiesce_candidates"] / max(1, split["quiesce_nodes"])
                print(f"{preset:9s} {budget:5d} {q} | {stats['evals'] / sec:.4g} | {stats['steps'] / sec:.4g} | "
                      f"{stats['positions'] / sec:.4g} | {stats['games'] / sec:.4g} | {split['main_nodes'] / moves:.1f} + "
                      f"{split['quiesce_nodes'] / moves:.1f} | {per_main:.1f} | {per_q:.2f} ({100.0 * per_q / max(per_main, 1e-9):.1f} %) | "
                      f"{sec:.2f}", flush=True)
    print(f"# wall time {time.perf_counter() - t_start:.1f} s")


if __name__ == "__main__":
    main()
