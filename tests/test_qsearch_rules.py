"""tests/_qsearch_rules.py - the recursive restatement the quiescence games are replayed through on the GPU box - checked on
the CPU (leaf values from the oracle): against tests/_search_rules.py at Q = 0, against a recursion without any pruning, on
hand-made positions for every branch of quiesce(), and for the condition that keeps the GPU tests from passing vacuously."""
import numpy as np
import pytest

# the (budget, Q) pairs tests/test_gpu_qsearch.py plays
GPU_CASES = [(25, 1), (25, 4), (25, 8), (150, 1), (150, 4), (150, 8)]


@pytest.fixture(scope="module")
def oracle_state(sp, oracle, net_blob):
    class OracleState:  # what Searcher asks of an NnueState: raw evals of a batch of records (kept: the searches below revisit
        def __init__(self):  # the same trees with other budgets and quiescence plies)
            self.known = {}

        def evaluate_once(self, recs):
            keys = [r.tobytes() for r in recs]
            new = [i for i, k in enumerate(keys) if k not in self.known]
            if new:
                oracle.use(net_blob("tame"), "tame")
                mail, stm = sp.positions_to_mailboxes(recs[new])
                for i, v in zip(new, oracle.eval_mailboxes(mail, stm)):
                    self.known[keys[i]] = int(v)
            return np.array([self.known[k] for k in keys], dtype=np.int32)

    return OracleState()


@pytest.fixture(scope="module")
def roots(sp):
    return sp.random_positions(16, seed=99, min_ply=20, max_ply=70, dfrc_every=2)


def test_without_quiescence_plies_it_is_the_plain_search(sp, oracle_state, roots):
    """Q = 0: move, score, depth and node count of _search_rules.Searcher.root on the same roots."""
    from _qsearch_rules import QSearcher
    from _search_rules import Searcher

    for budget in (1, 25, 90, 150):
        plain, restated = Searcher(sp, oracle_state, budget), QSearcher(sp, oracle_state, budget, 0)
        for rec in roots[:8]:
            word, score, _, depth = plain.root(rec)
            nodes = plain.nodes
            got = restated.root(rec)
            assert (word, score, depth) == (got[0], got[1], got[3])
            assert restated.nodes == nodes
        assert restated.quiesce_nodes == 0 and restated.main_nodes == restated.expanded == plain.expanded


@pytest.mark.parametrize("quiesce_plies", [1, 3])
def test_restated_quiescence_search_against_a_recursion_without_pruning(sp, oracle_state, roots, quiesce_plies):
    """The reference: full-width negamax to the depth the restated search reached whose depth-0 nodes are un-windowed quiescence
    maxima (max(stand, max over the candidates ...), in check without the stand). Alpha-beta is exact against it EXCEPT for the
    one thing the rules accept knowingly: the stand-pat cut-off is decided before the node is expanded, so a node IN CHECK whose
    static evaluation is at or above beta returns it although it has no stand pat. No recursion without a window can follow
    that (the outcome depends on beta), so the comparison is made in the two ways that are exact:
      * the restatement with that single decision made check-aware (QSearcher.stand_pat_cuts_unexpanded overridden, nothing
        else) must give the reference's root score, and a best move of it, at EVERY root;
      * the restatement AS SPECIFIED must do so at every root whose search never cut off a node in check by its stand pat, and
        then be the check-aware search node for node. Three late-game roots (few pieces, few checks) join the five random
        ones so that such roots exist at Q = 3 too: for every (budget, Q) at least one is asserted - at Q = 3 a 4-piece ending
        searched to depth 3 with 78 quiescence nodes among its 143 - and where the scores differ, the check-aware search must
        have expanded other nodes.
    Measured when this test was written (5 roots, budgets 25 / 90): Q = 1: 26 such cut-offs at one root move its score from 54
    to 123, the other roots (0 - 7 cut-offs) are exact; Q = 3: 3 - 160 cut-offs per root of the five, scores differ at three or four of them
    by 4 - 104 units; the late-game roots have 0 / 0 / 0 cut-offs at budget 25 and 47 / 1 / 0 at budget 90."""
    from _qsearch_rules import QSearcher
    from _search_rules import MATE

    class Counting(QSearcher):
        check_aware = False

        def __init__(self, *args):
            super().__init__(*args)
            self.in_check_cuts = 0

        def stand_pat_cuts_unexpanded(self, rec):
            if not self.sp.legal_moves(rec)[2]:
                return True
            self.in_check_cuts += 1
            return not self.check_aware

    class CheckAware(Counting):
        check_aware = True

    def quiesce(s, rec, stand, ply, q):
        if q == 0:
            return stand
        kids, values, in_check, order, _ = s.expand_quiesce(rec)
        if in_check and not order:
            return -(MATE - ply)
        below = [-quiesce(s, kids[i], -values[i], ply + 1, q - 1) for i in order]
        return max(below) if in_check else max([stand] + below)

    def minimax(s, rec, depth, ply):
        words, kids, values, in_check, order = s.expand(rec)
        if len(words) == 0:
            return -(MATE - ply) if in_check else 0
        if depth == 1:
            return max(-quiesce(s, kids[i], -values[i], ply + 1, quiesce_plies) for i in order)
        return max(-minimax(s, kids[i], depth - 1, ply + 1) for i in order)

    def unpruned(s, rec, depth):
        words, kids, values, _, _ = s.expand(rec)
        return [(-minimax(s, kids[i], depth - 1, 1) if depth > 1 else -quiesce(s, kids[i], -values[i], 1, quiesce_plies))
                for i in range(len(words))]

    late = sp.random_positions(24, seed=7, min_ply=120, max_ply=260, dfrc_every=0)[[3, 5, 6]]
    for budget in (25, 90):
        exact_as_specified = 0
        for rec in list(roots[:5]) + list(late):
            results = []
            for kind in (Counting, CheckAware):
                searcher = kind(sp, oracle_state, budget, quiesce_plies)
                word, score, _, depth = searcher.root(rec)
                nodes, cuts = searcher.nodes, searcher.in_check_cuts
                full = unpruned(searcher, rec, depth)
                best_move = full[list(searcher.expand(rec)[0]).index(word)] == max(full)
                results.append((score, max(full), best_move, nodes, cuts, depth))
            (score, want, best_move, nodes, cuts, depth), aware = results
            print(f"budget {budget} Q {quiesce_plies}: as specified depth {depth}, {nodes} nodes, score {score} (unpruned {want}), "
                  f"{cuts} stand-pat cut-offs of nodes in check; check-aware depth {aware[5]}, {aware[3]} nodes, score {aware[0]} "
                  f"(unpruned {aware[1]})")
            assert aware[0] == aware[1] and aware[2], (budget, quiesce_plies, aware)
            if cuts == 0:
                assert score == want and best_move and (score, nodes, depth) == (aware[0], aware[3], aware[5])
                exact_as_specified += 1
            elif (score, best_move) != (want, True):
                assert nodes != aware[3]
        assert exact_as_specified >= 1, (budget, quiesce_plies)


def test_branches_of_quiesce_on_hand_made_positions(sp, oracle_state):
    from _qsearch_rules import QSearcher, is_noisy
    from _search_rules import INF, MATE

    def fen(text):
        return sp.positions_from_fens([text])[0]

    # in check without an evasion (back-rank mate, black to move): the mate score of the node's ply, whatever the stand pat
    s = QSearcher(sp, oracle_state, 100, 4)
    mated = fen("R5k1/5ppp/8/8/8/8/8/4K3 b - - 0 1")
    assert s.quiesce(mated, 123, -INF, INF, 3, 2) == -(MATE - 3) and s.quiesce_nodes == 1
    # not in check, no noisy move (the start position): the stand pat, and still one expansion
    s = QSearcher(sp, oracle_state, 100, 4)
    start = fen("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1")
    assert s.quiesce(start, 17, -INF, INF, 2, 1) == 17 and (s.quiesce_nodes, s.nodes, s.candidates, s.legal) == (1, 1, 0, 20)
    # the horizon expands nothing; neither does a stand pat at or above beta
    s = QSearcher(sp, oracle_state, 100, 4)
    assert s.quiesce(start, -5, -INF, INF, 2, 0) == -5 and s.quiesce(start, 40, -INF, 40, 2, 3) == 40
    assert (s.quiesce_nodes, s.nodes, s.deepest_quiesce) == (0, 0, 0)
    # candidates: a quiet promotion offers its queen alone, a capturing one all four pieces; castling never; in check all evasions
    promo = fen("1n2k3/P7/8/8/8/8/8/R3K2R w KQ - 0 1")
    words, _, in_check = sp.legal_moves(promo)
    assert not in_check and sum(int(w) >> 14 == 2 for w in words) == 2   # both castlings are legal ...
    s = QSearcher(sp, oracle_state, 100, 4)
    _, values, _, order, n_legal = s.expand_quiesce(promo)
    got = sorted(int(words[i]) for i in order)
    a7, a8, b8 = 48, 56, 57
    quiet_queen = a7 | (a8 << 6) | (3 << 12) | 0xC000
    captures = [a7 | (b8 << 6) | (pt << 12) | 0xC000 for pt in range(4)]
    assert got == sorted([quiet_queen] + captures) and n_legal == len(words) > 5
    assert not any(is_noisy(promo, w) for w in words if int(w) >> 14 == 2)   # ... and never candidates
    assert not is_noisy(promo, a7 | (a8 << 6) | (2 << 12) | 0xC000) and is_noisy(promo, captures[0])
    ep = fen("4k3/8/8/3pP3/8/8/8/4K3 w - d6 0 2")
    ep_words = [int(w) for w in sp.legal_moves(ep)[0]]
    assert [w for w in ep_words if is_noisy(ep, w)] == [36 | (43 << 6) | 0x4000]
    checked = fen("4k3/8/8/8/8/8/4r3/4K3 w - - 0 1")   # in check: every evasion is a candidate, quiet or not
    ev_words, _, ev_check = sp.legal_moves(checked)
    s = QSearcher(sp, oracle_state, 100, 4)
    assert ev_check and len(s.expand_quiesce(checked)[3]) == len(ev_words) >= 2
    # in check there is no stand pat: the value is the best evasion's, even below a huge stand (window open)
    s = QSearcher(sp, oracle_state, 100, 1)
    kids, values, _, order, _ = s.expand_quiesce(checked)
    assert s.quiesce(checked, 30000, -INF, INF, 1, 1) == values[order[0]] < 30000
    # out of check the stand pat is a lower bound
    s = QSearcher(sp, oracle_state, 100, 1)
    kids, values, _, order, _ = s.expand_quiesce(promo)
    assert s.quiesce(promo, 30000, -INF, INF, 1, 1) == 30000
    assert s.quiesce(promo, -30000, -INF, INF, 1, 1) == values[order[0]]


def test_the_gpu_cases_exercise_quiescence(sp, oracle_state, roots):
    """So that tests/test_gpu_qsearch.py cannot pass vacuously: over 16 random roots and for each (budget, Q) it plays, the
    restated search must (a) expand quiescence nodes in at least half of the searches, (b) reach quiescence ply min(Q, 2)
    somewhere, and (c) choose another move than the Q = 0 search at one root at least."""
    from _qsearch_rules import QSearcher
    from _search_rules import Searcher

    for budget, q in GPU_CASES:
        plain, restated = Searcher(sp, oracle_state, budget), QSearcher(sp, oracle_state, budget, q)
        with_nodes = differ = 0
        for rec in roots:
            before = restated.quiesce_nodes
            word = restated.root(rec)[0]
            with_nodes += restated.quiesce_nodes > before
            differ += word != plain.root(rec)[0]
        print(f"budget {budget} Q {q}: {with_nodes}/16 searches with quiescence nodes, deepest ply {restated.deepest_quiesce}, "
              f"{differ}/16 moves differ, {restated.quiesce_nodes} of {restated.expanded} nodes, candidates "
              f"{restated.candidates} of {restated.legal} legal moves")
        assert with_nodes >= 8 and restated.deepest_quiesce >= min(q, 2) and differ >= 1, (budget, q)
