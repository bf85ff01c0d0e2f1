"""A/B of the opt-in refresh tables (spx_acc_reserve_refresh_tables) in one process: A = no tables, B = tables, alternated
--rounds times each; median and spread of every figure.
  (a) the secondary.incremental shape of bench.py (incremental_leg): 65 536 games, the forward-and-back ply walk through
      spx_acc_update_eval_device_async; in B game g's two slots are bound to table g. Updates + evals/s and the spx_profile_*
      "ft" interval (update kernel + rebuild pass) per ply.
  (b) the selfplay_search_leg shape (4 096 seats, 64-node search) with and without SPX_SELFPLAY_REFRESH_TABLES: leaf evals/s.
  (c) for both: the table's share of the rebuilds and the piece-square rows it saved (spx_debug_refresh_table_stats).
Usage: python tools/gpu_refresh_tables_ab.py [--rounds 5] [--preset tame] [--skip-selfplay]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rocm_version():
    try:
        return open("/opt/rocm/.info/version").read().strip()
    except OSError:
        return subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()[0:1]


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "spread_pct": 100.0 * (max(xs) - min(xs)) / statistics.median(xs) if statistics.median(xs) else 0.0}


class Walk:
    """incremental_leg of bench.py on one context (same boards, same walk); tables=True binds game g's slots to table g."""

    def __init__(self, sp, torch, net, games, chain, tables):
        from stormphrax_amd import _lib

        self.torch, self.lib, self._lib = torch, _lib.load(), _lib
        self.st = sp.NnueState(net, device=0, max_batch=games)
        self.games = games
        self.boards = []
        quarter = games // 4
        for k in range(chain):
            t = torch.empty((games, 32), dtype=torch.uint8, device="cuda")
            for q, base in enumerate((10, 30, 60, 100)):
                cnt = quarter if q < 3 else games - 3 * quarter
                self.st.random_positions_device(t[q * quarter:].data_ptr(), cnt, seed=4242 + q, min_ply=base + k, max_ply=base + k,
                                                dfrc_every=4)
            self.boards.append(t)
        self.st.reserve_slots(2 * games)
        if tables:
            self.st.reserve_refresh_tables(games)
            g = np.arange(games, dtype=np.uint32)
            self.st.bind_refresh_tables(np.concatenate([g, g + games]), np.concatenate([g, g]))
        self.slots = [torch.arange(games, dtype=torch.int32, device="cuda"),
                      torch.arange(games, 2 * games, dtype=torch.int32, device="cuda")]
        self.outs = [torch.empty(games, dtype=torch.int32, device="cuda") for _ in range(2)]
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.lib.spx_acc_refresh_device(self.st._h, self.boards[0].data_ptr(), self.slots[0].data_ptr(), games, stream))
        torch.cuda.synchronize()
        self.L, self.no = chain, 0

    def board_index(self, step):
        k = step % (2 * self.L - 2)
        return k if k < self.L else 2 * self.L - 2 - k

    def step(self):
        s_ = self.no
        self._lib.check(self.lib.spx_acc_update_eval_device_async(
            self.st._h, self.slots[s_ & 1].data_ptr(), self.slots[(s_ + 1) & 1].data_ptr(),
            self.boards[self.board_index(s_ + 1)].data_ptr(), self.games, self.outs[s_ & 1].data_ptr(), None))
        self.no = s_ + 1

    def sync(self):
        self.st.synchronize()
        self.torch.cuda.synchronize()

    def measure(self, seconds):
        for _ in range(40):  # warm-up
            self.step()
        self.sync()
        self.st.refresh_table_stats()
        steps = 0
        self.st.profile_begin(4096)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds and steps < 4000:
            for _ in range(20):
                self.step()
            steps += 20
            self.sync()
        elapsed = time.perf_counter() - t0
        _, ft_ms, _, calls = self.st.profile_end()
        stats = self.st.refresh_table_stats()
        full = self.torch.empty(self.games, dtype=self.torch.int32, device="cuda")
        self.st.evaluate_once_device(self.boards[self.board_index(self.no)].data_ptr(), self.games, full.data_ptr(),
                                     self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        exact = bool(self.torch.equal(full, self.outs[(self.no - 1) & 1]))
        return {"rate": self.games * steps / elapsed, "ft_ms": ft_ms / max(calls, 1), "exact": exact, "stats": stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preset", default="tame")
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--seats", type=int, default=4096)
    ap.add_argument("--skip-selfplay", action="store_true")
    args = ap.parse_args()

    import torch

    import stormphrax_amd as sp

    net = sp.Network(sp.synthetic_net_bytes(args.preset))
    t_start = time.perf_counter()
    print(f"# refresh tables A/B  rocm {rocm_version()}  torch {torch.__version__}  preset {args.preset}  rounds {args.rounds}")
    walks = {"A": Walk(sp, torch, net, args.games, 6, False), "B": Walk(sp, torch, net, args.games, 6, True)}
    inc = {"A": [], "B": []}
    for r in range(args.rounds):
        for mode in ("A", "B"):
            m = walks[mode].measure(args.seconds)
            inc[mode].append(m)
            s = m["stats"]
            print(f"(a) round {r} {mode}: {m['rate']:.4g} updates+evals/s  ft {m['ft_ms'] * 1e3:.1f} us/ply  exact {m['exact']}  "
                  f"rebuilt {s['rebuilt']} served {s['served']} rows applied {s['rows_applied']} / scratch {s['scratch_rows']}")
    for w in walks.values():
        w.st.close()
    print("(a) incremental, 65 536 games, pipelined forward-and-back walk:")
    for mode in ("A", "B"):
        rate, ft = summary([m["rate"] for m in inc[mode]]), summary([m["ft_ms"] * 1e3 for m in inc[mode]])
        print(f"    {mode}: updates+evals/s median {rate['median']:.4g} (min {rate['min']:.4g}, max {rate['max']:.4g}, spread "
              f"{rate['spread_pct']:.1f} %)  ft interval median {ft['median']:.1f} us/ply (spread {ft['spread_pct']:.1f} %)  "
              f"all exact {all(m['exact'] for m in inc[mode])}")
    sb = [m["stats"] for m in inc["B"]]
    rebuilt, served = sum(s["rebuilt"] for s in sb), sum(s["served"] for s in sb)
    applied, scratch = sum(s["rows_applied"] for s in sb), sum(s["scratch_rows"] for s in sb)
    print(f"(c) incremental B: table served {served} of {rebuilt} rebuilds ({100.0 * served / max(1, rebuilt):.1f} %); psq rows "
          f"applied {applied} vs {scratch} from scratch ({100.0 * (1 - applied / max(1, scratch)):.1f} % saved, "
          f"{applied / max(1, served):.2f} vs {scratch / max(1, served):.2f} per served rebuild)")

    if not args.skip_selfplay:
        sp_runs = {"A": [], "B": []}
        for r in range(args.rounds):
            for mode in ("A", "B"):
                with sp.NnueState(net, device=0, max_batch=args.seats * 64) as st:
                    stats = st.selfplay(n_games=args.seats, target_games=args.seats, out_path=None, max_plies=300, dfrc=True,
                                        temperature_cp=0, seed=1, search_nodes=64, refresh_tables=(mode == "B"))
                    rt = st.refresh_table_stats()
                sp_runs[mode].append((stats["evals"] / stats["seconds"], rt))
                print(f"(b) round {r} {mode}: {stats['evals'] / stats['seconds']:.4g} leaf evals/s  ({stats['seconds']:.2f} s)  "
                      f"rebuilt {rt['rebuilt']} served {rt['served']} rows applied {rt['rows_applied']} / scratch {rt['scratch_rows']}")
        print(f"(b) self-play, {args.seats} seats, 64-node search:")
        for mode in ("A", "B"):
            s = summary([x[0] for x in sp_runs[mode]])
            print(f"    {mode}: leaf evals/s median {s['median']:.4g} (min {s['min']:.4g}, max {s['max']:.4g}, spread {s['spread_pct']:.1f} %)")
        sb = [x[1] for x in sp_runs["B"]]
        rebuilt, served = sum(s["rebuilt"] for s in sb), sum(s["served"] for s in sb)
        applied, scratch = sum(s["rows_applied"] for s in sb), sum(s["scratch_rows"] for s in sb)
        print(f"(c) self-play B: table served {served} of {rebuilt} rebuilds ({100.0 * served / max(1, rebuilt):.1f} %); psq rows "
              f"applied {applied} vs {scratch} from scratch ({100.0 * (1 - applied / max(1, scratch)):.1f} % saved)")
    print(f"# wall time {time.perf_counter() - t_start:.1f} s")


if __name__ == "__main__":
    main()
