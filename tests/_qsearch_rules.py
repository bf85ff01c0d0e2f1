"""Plain-Python restatement of the live search WITH QUIESCENCE (SPX_SELFPLAY_QUIESCE_PLIES; the rules are with
SearchStepParams in stormphrax_amd/csrc/spx_kernels.h; the role is qsearch, src/search.cpp:1451-1640). TEST INFRASTRUCTURE,
built on tests/_search_rules.py: the literal recursion, one node at a time, nothing shared with the device's quiescence frames
(spx_search_step_kernel<true>) or with the move generator's quiescence mode - the candidates of a quiescence node are filtered
HERE, from the move word and the parent's occupancy:

  noisy(move)    = not castling, and (en passant, or promotion to a queen, or the target square is occupied)
                                                                                  (Position::isNoisy, position.cpp:683-689)
  search(node, depth, alpha, beta, ply)
                 = as in _search_rules, except at depth 1: every child c is worth -quiesce(c, -value(c), -beta, -alpha,
                   ply + 1, Q), fail-soft with the cut-off at alpha >= beta like the deeper levels
  quiesce(c, stand, a, b, ply, q)              c has NOT been expanded; stand = net(c) clamped, from c's mover
                 = stand when q == 0 (horizon) or stand >= b (stand-pat cut-off, decided without expanding c); else c is
                   expanded in quiescence mode (one node): in check every legal move is a candidate, else the noisy ones;
                   in check without a candidate -(MATE - ply); in check best = -INF, else best = stand and a = max(a, stand)
                   (no candidate: stand - stalemate is not detected); the candidates by (value descending, move word
                   ascending), x = -quiesce(child, -value(child), -b, -a, ply + 1, q - 1), fail-soft, stop at a >= b
  root           : as in _search_rules (iteration 1 is the depth-1 line above with the window (-INF, -alpha))

`verify_qsearch_file` is `_search_rules.verify_search_file` with this searcher."""
import ctypes

import numpy as np

from _datagen_rules import K_SCORE_WIN, VERIFICATION_SCORE_LIMIT, clamp_static, classical_material, parse_games, replay_game
from _search_rules import INF, LEVELS, MATE, Searcher

MAX_QUIESCE_PLIES = 8   # kQuiesceMaxPlies


def is_noisy(rec, word):
    """Position::isNoisy of the move `word` (viriformat) at the position `rec`."""
    word = int(word)
    kind, to = word >> 14, (word >> 6) & 63   # 0 normal, 1 en passant, 2 castling, 3 promotion (viriformat.cpp:37-52)
    if kind == 2:
        return False
    if kind == 1:
        return True
    if kind == 3 and ((word >> 12) & 3) == 3:
        return True
    return bool((int(rec["occupancy"]) >> to) & 1)


class QSearcher(Searcher):
    def __init__(self, sp, st, budget, quiesce_plies):
        super().__init__(sp, st, budget)
        self.q = quiesce_plies
        self.qcache = {}
        self.main_nodes = 0        # expansions of all searches: main nodes ...
        self.quiesce_nodes = 0     # ... and quiescence nodes
        self.deepest_quiesce = 0   # deepest quiescence ply expanded (1 = the child of a depth-1 node)
        self.candidates = 0        # candidates / legal moves of the quiescence nodes expanded
        self.legal = 0
        self.searches = 0          # root() calls, and those that expanded a quiescence node
        self.searches_with_quiesce = 0
        self.largest_search = 0    # most nodes one search expanded

    def expand(self, rec):
        self.main_nodes += 1
        return super().expand(rec)

    def expand_quiesce(self, rec):
        key = rec.tobytes()
        hit = self.qcache.get(key)
        if hit is None:
            words, kids, in_check = self.sp.legal_moves(rec)
            keep = [i for i in range(len(words)) if in_check or is_noisy(rec, words[i])]
            values = {}
            if keep:
                raw = self.st.evaluate_once(kids[keep])
                values = {i: clamp_static(-int(v)) for i, v in zip(keep, raw)}
                if len(self.leaves) < 200000:
                    self.leaves.extend((kids[i].tobytes(), int(v)) for i, v in list(zip(keep, raw))[::7])
            order = sorted(keep, key=lambda i: (-values[i], int(words[i])))
            hit = (kids, values, bool(in_check), order, len(words))
            self.qcache[key] = hit
        self.nodes += 1
        self.expanded += 1
        self.quiesce_nodes += 1
        self.candidates += len(hit[3])
        self.legal += hit[4]
        return hit

    def stand_pat_cuts_unexpanded(self, rec):
        """The rule as specified: ALWAYS - c's check status is unknown before its expansion, and a node in check whose static
        evaluation is at or above beta returns it although it has no stand pat (accepted). tests/test_qsearch_rules.py
        overrides this one decision to measure what the acceptance costs against a search without pruning."""
        return True

    def quiesce(self, rec, stand, a, b, ply, q):
        if q == 0:
            return stand
        if stand >= b and self.stand_pat_cuts_unexpanded(rec):
            return stand
        self.deepest_quiesce = max(self.deepest_quiesce, self.q - q + 1)
        kids, values, in_check, order, _ = self.expand_quiesce(rec)
        if in_check and not order:
            return -(MATE - ply)
        if in_check:
            best = -INF
        else:
            best = stand
            a = max(a, stand)
        for i in order:
            x = -self.quiesce(kids[i], -values[i], -b, -a, ply + 1, q - 1)
            if x > best:
                best = x
            if x > a:
                a = x
            if a >= b:
                break
        return best

    def search(self, rec, depth, alpha, beta, ply):
        words, kids, values, in_check, order = self.expand(rec)
        if len(words) == 0:
            return -(MATE - ply) if in_check else 0
        best = -INF
        for i in order:
            if depth >= 2:
                v = -self.search(kids[i], depth - 1, -beta, -alpha, ply + 1)
            else:
                v = -self.quiesce(kids[i], -values[i], -beta, -alpha, ply + 1, self.q)
            if v > best:
                best = v
            if v > alpha:
                alpha = v
            if alpha >= beta:
                break
        return best

    def root(self, rec):
        """-> (move word, score of the mover, child record, depth) of the move the driver must play at `rec` (which has legal
        moves)."""
        self.cache.clear()
        self.qcache.clear()
        self.nodes = 0
        quiesce_before = self.quiesce_nodes
        words, kids, values, _, order = self.expand(rec)
        depth, best_idx, best = 0, None, -INF
        while True:
            depth += 1
            alpha, best, prev = -INF, -INF, best_idx
            for i in (order if prev is None else [prev] + [k for k in order if k != prev]):
                if depth >= 2:
                    v = -self.search(kids[i], depth - 1, -INF, -alpha, 1)
                else:
                    v = -self.quiesce(kids[i], -values[i], -INF, -alpha, 1, self.q)
                if v > best:
                    best, best_idx = v, i
                if v > alpha:
                    alpha = v
            if self.nodes >= self.budget or depth >= LEVELS or abs(best) > K_SCORE_WIN:
                break
        self.searches += 1
        self.searches_with_quiesce += self.quiesce_nodes > quiesce_before
        self.largest_search = max(self.largest_search, self.nodes)
        return int(words[best_idx]), best, kids[best_idx], depth


def verify_qsearch_file(sp, st, oracle, blob, max_plies, budget, quiesce_plies, tally=None, plain=None):
    """-> (plies checked, the QSearcher that replayed them, deepest iteration seen). `oracle.use(...)` must have been called
    for the net `st` runs. plain: optional list that receives, per ply, whether the search WITHOUT quiescence
    (_search_rules.Searcher, same budget) would have played another move."""
    positions, n_games = sp.viri_expand(blob)
    games = parse_games(blob)
    assert len(games) == n_games and sum(len(g[1]) for g in games) == len(positions)
    wdl = oracle.lib.spxo_wdl_normalize
    wdl.argtypes, wdl.restype = [ctypes.c_int32, ctypes.c_int32], ctypes.c_int32

    def normalize(score, material):
        return int(wdl(int(score), int(material)))

    searcher = QSearcher(sp, st, budget, quiesce_plies)
    without = Searcher(sp, st, budget) if plain is not None else None
    start = checked = deepest = 0
    for gi, (_, moves, scores, outcome) in enumerate(games):
        n = len(moves)
        assert n >= 1
        before = positions[start:start + n]
        assert np.array_equal(before["eval"], scores) and np.all(before["wdl"] == outcome)
        mover = []
        last_child = None
        for k in range(n):
            word, score, child, depth = searcher.root(before[k])
            assert word == int(moves[k]), (gi, k, word, int(moves[k]))
            if without is not None:
                plain.append(without.root(before[k])[0] != word)
            if k + 1 < n:
                assert child.tobytes()[:28] == before[k + 1].tobytes()[:28], (gi, k)
            mover.append(score)
            last_child = child
            deepest = max(deepest, depth)
            if k == 0:  # the first search doubles as the opening's verification search (datagen.cpp:176-190)
                white = not (int(before[0]["stm_ep"]) & 0x80)
                norm = normalize(score if white else -score, int(classical_material(before[:1])[0]))
                assert abs(norm) <= VERIFICATION_SCORE_LIMIT, (gi, norm)
        replies, _, in_check = sp.legal_moves(last_child)
        want_outcome, stop, recorded = replay_game(before, last_child, mover, normalize, max_plies,
                                                   len(replies) == 0 and bool(in_check), len(replies) > 0, tally)
        assert (want_outcome, stop) == (outcome, n), (gi, want_outcome, outcome, stop, n)
        assert recorded == [int(s) for s in scores], gi
        checked += n
        start += n
    # the leaves the restated searches saw (GPU, from scratch) against the CPU oracle
    sample = searcher.leaves[:: max(1, len(searcher.leaves) // 4096)]
    recs = np.frombuffer(b"".join(r for r, _ in sample), dtype=sp.PACKED_DTYPE)
    mail, stm = sp.positions_to_mailboxes(recs)
    assert np.array_equal(oracle.eval_mailboxes(mail, stm), np.array([v for _, v in sample])), "GPU evals differ from the CPU oracle"
    return checked, searcher, deepest
