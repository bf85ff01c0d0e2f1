#!/usr/bin/env python3
"""Default path A/B against the PARENT COMMIT on one box: secondary.config4_selfplay_search of bench.py (selfplay_search_leg alone)
and the headline, parent and this tree alternated --rounds times each; per figure the runs, min, max and spread, and whether
this tree's runs lie inside the parent's own spread.
The parent runs from a checkout of its own (its library under its own Python package and bench.py, so that neither side sees
the other's ctypes table):
    git worktree add variants/parent_tree HEAD~1 && (cd variants/parent_tree && python -c "import __graft_entry__ as g; g.build()")
    python tools/gpu_default_path_ab.py [--parent variants/parent_tree] [--rounds 3] [--no-headline] [--tree-first]
--tree-first swaps the order inside a round: the headline's code is usually the same on both sides, so its difference, and how
it moves with the order, shows what the position in the round alone is worth."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEG = ("import json, sys; sys.path.insert(0, '.'); import bench, stormphrax_amd as sp; "
       "print(json.dumps(bench.selfplay_search_leg(sp, sp.Network(sp.synthetic_net_bytes('tame')), 0)))")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "variants", "parent_tree"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--tree-first", action="store_true")
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "tree": ROOT}
    if args.tree_first:
        trees = dict(reversed(list(trees.items())))
    figures = {"config4_selfplay_search": {"parent": [], "tree": []}, "headline": {"parent": [], "tree": []}}
    env = {k: v for k, v in os.environ.items() if k != "SPX_LIB"}
    for r in range(args.rounds):
        for name, cwd in trees.items():
            p = subprocess.run([sys.executable, "-c", LEG], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"round {r} {name}: search leg failed ({p.returncode}): {p.stderr[-600:]}")
            j = json.loads(p.stdout.strip().splitlines()[-1])
            figures["config4_selfplay_search"][name].append(j["value"])
            print(f"round {r} {name:6s} config4_selfplay_search {j['value']:.5e} leaf evals/s  ({j['seconds']:.2f} s, "
                  f"{j['nodes_expanded']} nodes, {j['positions']} positions, {j['evals']} leaves)", flush=True)
            if args.no_headline:
                continue
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "10", "--no-cpu-baseline",
                                "--no-secondary", "--no-wide"], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"round {r} {name}: bench.py failed ({p.returncode}): {p.stderr[-600:]}")
            j = json.loads(p.stdout.strip().splitlines()[-1])
            figures["headline"][name].append(j["value"])
            print(f"round {r} {name:6s} headline {j['value']:.5e} {j.get('unit', '')}", flush=True)
    for what, runs in figures.items():
        if not runs["parent"]:
            continue
        lo, hi = min(runs["parent"]), max(runs["parent"])
        for name in ("parent", "tree"):
            v = runs[name]
            print(f"{what} {name:6s} min {min(v):.5e} max {max(v):.5e} spread {100 * (max(v) - min(v)) / min(v):.2f} %")
        inside = [lo <= v <= hi for v in runs["tree"]]
        print(f"{what}: {sum(inside)} of {len(inside)} runs of this tree inside the parent's spread; below its minimum: "
              f"{[f'{100 * (v / lo - 1):+.2f} %' for v in runs['tree'] if v < lo]}, above its maximum: "
              f"{[f'{100 * (v / hi - 1):+.2f} %' for v in runs['tree'] if v > hi]}")


if __name__ == "__main__":
    main()
