"""tests/_qprune_rules.py - the restatement the pruned quiescence games are replayed through on the GPU box - checked on the CPU
(leaf values from the oracle): with every pruning branch switched off it is tests/_qsearch_rules.QSearcher node for node;
hand-made positions for each branch of the node; and the conditions that keep tests/test_gpu_qprune.py from passing vacuously."""
import numpy as np
import pytest

from test_qsearch_rules import oracle_state, roots  # noqa: F401  (fixtures: oracle evaluations kept per record, 16 random roots)

# the (budget, Q) pairs tests/test_gpu_qprune.py plays
GPU_CASES = [(25, 1), (25, 4), (25, 8), (150, 1), (150, 4), (150, 8)]


def test_with_every_branch_off_it_is_the_unpruned_search(sp, oracle_state, roots):
    from _qprune_rules import PrunedQSearcher
    from _qsearch_rules import QSearcher

    for budget, q in ((25, 2), (90, 4)):
        plain, off = QSearcher(sp, oracle_state, budget, q), PrunedQSearcher(sp, oracle_state, budget, q, branches=())
        for rec in roots[:6]:
            a, b = plain.root(rec), off.root(rec)
            assert (a[0], a[1], a[3]) == (b[0], b[1], b[3]) and plain.nodes == off.nodes
        assert (plain.expanded, plain.quiesce_nodes, plain.candidates, plain.legal, plain.deepest_quiesce) == \
               (off.expanded, off.quiesce_nodes, off.candidates, off.legal, off.deepest_quiesce)
        assert not any(n for name, n in off.taken.items() if name != "first evasion searched as a loss")   # (an observation)


def test_branches_of_the_pruned_node_on_hand_made_positions(sp, oracle_state):
    from _qprune_rules import ALL_BRANCHES, FP_MARGIN, PrunedQSearcher
    from _search_rules import INF, MATE

    def fen(text):
        return sp.positions_from_fens([text])[0]

    def searcher(q=1, **kw):
        return PrunedQSearcher(sp, oracle_state, 100, q, **kw)

    # futility by the generator: the only noisy move, an en passant that c7 takes back, fails see(1). With alpha far above the
    # stand pat the node is expanded in mode 3: nothing is generated, one move was dropped, so best = stand + 142
    ep = fen("4k3/2p5/8/3pP3/8/8/8/4K3 w - d6 0 1")
    s = searcher()
    assert s.quiesce(ep, 10, 500, INF, 1, 1) == 10 + FP_MARGIN
    assert (s.quiesce_nodes, s.candidates, s.taken["lifted by dropped moves"]) == (1, 0, 1)
    # ... with the window open it is mode 2: the capture passes see(-81), is a candidate and is searched (q = 1: worth its value)
    s = searcher()
    _, values, _, order, _, pruned = s.expand_pruned(ep, False)
    assert len(order) == 1 and pruned == 0
    assert searcher().quiesce(ep, 10, -INF, INF, 1, 1) == max(10, values[order[0]])
    # the generator's see(-81) filter: a queen that takes a defended pawn is never a candidate, the stand pat stays
    losing = fen("4k3/8/3p4/4p3/8/8/8/4QK2 w - - 0 1")
    s = searcher()
    assert s.quiesce(losing, 33, -INF, INF, 1, 1) == 33 and (s.candidates, s.taken["generator see"]) == (0, 1)
    assert len(searcher(branches=()).expand_pruned(losing, False)[3]) == 1
    # futility after alpha rose: stand so low that the node is entered in mode 2 (fut > alpha); the first candidate's value lifts
    # alpha above fut, and the equal exchange (pawn takes defended pawn: see(-81) but not see(1)) that comes later is skipped
    # without counting as searched
    rose = fen("4k3/2p5/3p2r1/4P3/8/8/6R1/4K3 w - - 0 1")   # Rxg6 wins a rook; exd6 is answered by cxd6
    s = searcher()
    kids, values, in_check, order, flags, _ = s.expand_pruned(rose, False)
    assert not in_check and len(order) == 2 and [bool(flags[i] & 2) for i in order] == [True, False]
    stand = -20000
    assert stand + FP_MARGIN < values[order[0]]
    s = searcher()
    assert s.quiesce(rose, stand, -INF, INF, 1, 1) == values[order[0]] and s.taken["futility after alpha rose"] == 1
    off = searcher(branches=("generator see", "generator futility"))
    assert off.quiesce(rose, stand, -INF, INF, 1, 1) == values[order[0]] and off.taken["futility after alpha rose"] == 0
    # the cap out of check: three winning captures, two searched (q = 1: without a node of their own), the third never looked at
    three = fen("4k3/8/8/1q1r1n2/P1P1P1P1/8/8/4K3 w - - 0 1")
    s = searcher(q=2)
    kids, values, _, order, flags, _ = s.expand_pruned(three, False)
    assert len(order) >= 3 and all(flags[i] & 2 for i in order)
    s = searcher(q=2)
    s.quiesce(three, -20000, -INF, INF, 1, 2)
    assert s.taken["cap out of check"] == 1
    nocap = searcher(q=2, branches=("generator see", "generator futility"))
    nocap.quiesce(three, -20000, -INF, INF, 1, 2)
    assert nocap.taken["cap"] == 0 and nocap.quiesce_nodes >= s.quiesce_nodes
    # in check: the first evasion is always searched (best is still a loss); after it quiet evasions are skipped, an evasion
    # capture that loses material is skipped, and the cap holds
    checked = fen("4k3/8/8/3Q4/8/8/8/r3K3 w - - 0 1")   # Ra1+: king moves, and the queen can interpose on d1 (and lose herself)
    s = searcher()
    kids, values, in_check, order, flags, pruned = s.expand_pruned(checked, False)
    assert in_check and pruned == 0 and len(order) == len(sp.legal_moves(checked)[0]) >= 4
    assert any(not flags[i] & 1 for i in order) and not any(flags[i] & 4 for i in order)
    s = searcher()
    assert s.quiesce(checked, 0, -INF, INF, 1, 1) == values[order[0]]
    assert s.taken["first evasion searched as a loss"] == 1 and s.taken["quiet evasion"] == len(order) - 1
    def calls(q=1, **kw):
        """A searcher that counts its quiesce() calls: the node itself plus one per candidate searched."""
        class Counting(PrunedQSearcher):
            n_calls = 0

            def quiesce(self, *args):
                self.n_calls += 1
                return super().quiesce(*args)

        return Counting(sp, oracle_state, 100, q, **kw)

    without = lambda name: tuple(b for b in ALL_BRANCHES if b != name)   # noqa: E731
    # a losing evasion capture: Nd3+ is defended by e4, so Qxd3 loses the queen (noisy, see(-81) false). With the oracle's values
    # the king move e1e2 comes first and is searched (best is a loss until then); Qxd3 comes second and is skipped - not as a quiet
    # move but by its SEE bit; the two quiet king moves after it are skipped as quiet evasions. One candidate searched in all.
    lose = fen("4k3/8/8/8/4p3/3n4/8/3QK3 w - - 0 1")
    words = [int(w) for w in sp.legal_moves(lose)[0]]
    qxd3 = 3 | (19 << 6)
    s = calls()
    kids, values, in_check, order, flags, _ = s.expand_pruned(lose, False)
    assert in_check and len(order) == 4 and words[order[1]] == qxd3 and flags[order[1]] == 4 and words[order[0]] == 4 | (12 << 6)
    assert all(flags[i] == 1 for i in order if i != order[1])   # the king moves: quiet, see(-81) holds
    s = calls()
    assert s.quiesce(lose, 0, -INF, INF, 1, 1) == values[order[0]]
    assert (s.taken["losing evasion"], s.taken["quiet evasion"], s.taken["first evasion searched as a loss"], s.n_calls) == (1, 2, 1, 2)
    # the branch off: the queen sacrifice is searched too (one more call), which makes two searched - the cap stops the node
    # before the quiet king moves are looked at
    off = calls(branches=without("losing evasion"))
    assert off.quiesce(lose, 0, -INF, INF, 1, 1) == values[order[0]]
    assert (off.taken["losing evasion"], off.taken["quiet evasion"], off.taken["cap in check"], off.n_calls) == (0, 0, 1, 3)
    # the cap in check: Nd3+ is undefended and four pieces can take it (c2, Rd1, Bf1, Nb2: noisy, see(1) holds), two king moves are
    # quiet. The best two candidates are searched - the first while best is a loss, the second as the first "not a loss" one -
    # and the third candidate, another capture that passes every test, is never looked at
    capped = fen("4k3/8/8/8/8/3n4/1NP5/3RKB2 w - - 0 1")
    s = calls()
    kids, values, in_check, order, flags, _ = s.expand_pruned(capped, False)
    assert in_check and len(order) == 6 and sorted(flags[i] for i in order) == [1, 1, 7, 7, 7, 7]
    assert [flags[i] for i in order[:3]] == [7, 7, 7]   # (with the oracle's values three captures lead the order)
    s = calls()
    assert s.quiesce(capped, 0, -INF, INF, 1, 1) == values[order[0]]
    assert (s.taken["cap in check"], s.taken["cap"], s.taken["quiet evasion"], s.n_calls) == (1, 1, 0, 3)
    off = calls(branches=without("cap"))   # the cap off: all four captures are searched, the quiet king moves skipped
    assert off.quiesce(capped, 0, -INF, INF, 1, 1) == values[order[0]]
    assert (off.taken["cap"], off.taken["quiet evasion"], off.n_calls) == (0, 2, 5)
    # ... and the node counts differ where the candidates have plies left (Q = 2: a searched candidate above alpha is expanded)
    deep, deep_off = calls(q=2), calls(q=2, branches=without("cap"))
    deep.quiesce(capped, 0, -INF, INF, 1, 2)
    deep_off.quiesce(capped, 0, -INF, INF, 1, 2)
    print(f"cap in check at Q = 2: {deep.quiesce_nodes} quiescence nodes with the cap, {deep_off.quiesce_nodes} without")
    assert deep.taken["cap in check"] >= 1 and deep.quiesce_nodes <= deep_off.quiesce_nodes and deep.n_calls < deep_off.n_calls
    # mate in check is still mate, whatever the flags
    mated = fen("R5k1/5ppp/8/8/8/8/8/4K3 b - - 0 1")
    assert searcher().quiesce(mated, 123, -INF, INF, 3, 2) == -(MATE - 3)


def test_the_gpu_cases_exercise_pruning(sp, oracle_state, roots):
    """So that tests/test_gpu_qprune.py cannot pass vacuously. Over the 16 fixed roots and the (budget, Q) pairs it plays: the
    pruned search expands strictly fewer quiescence nodes IN SUM than the unpruned one (alpha-beta is not monotone per root: the
    per-root figures are printed, the sum asserted); every branch of the node is taken at least once over the grid; and at one
    root at least the pruned search plays another move than the unpruned one."""
    from _qprune_rules import PrunedQSearcher
    from _qsearch_rules import QSearcher

    taken, differ, total_pruned, total_plain = {}, 0, 0, 0
    for budget, q in GPU_CASES:
        plain, pruned = QSearcher(sp, oracle_state, budget, q), PrunedQSearcher(sp, oracle_state, budget, q)
        per_root = []
        for rec in roots:
            before = (plain.quiesce_nodes, pruned.quiesce_nodes)
            differ += plain.root(rec)[0] != pruned.root(rec)[0]
            per_root.append((plain.quiesce_nodes - before[0], pruned.quiesce_nodes - before[1]))
        print(f"budget {budget} Q {q}: quiescence nodes unpruned / pruned per root {per_root}; sums {plain.quiesce_nodes} / "
              f"{pruned.quiesce_nodes}; candidates {plain.candidates} / {pruned.candidates}; {pruned.taken}")
        total_plain += plain.quiesce_nodes
        total_pruned += pruned.quiesce_nodes
        for name, n in pruned.taken.items():
            taken[name] = taken.get(name, 0) + n
    print(f"sum over the grid: {total_plain} unpruned, {total_pruned} pruned quiescence nodes; {differ} moves differ; {taken}")
    assert total_pruned < total_plain
    assert all(n > 0 for n in taken.values()), taken
    assert differ >= 1
